// Speech features for a ragged batch of waveforms: MFCC (egs/ema/voc1/local/predict_ema.py:32-33, librosa 0.8.1's feature.mfcc) and the
// log-mel filterbank (articulatory/bin/preprocess.py:58-82).  STFT = frame gather + one GEMM against the mel loss's windowed DFT matrix on
// the exact-fp32 conv kernels with split-K off; the power or magnitude and the filterbank are one fused pass over the triangles (the padded
// filterbank GEMM of the mel loss multiplies mostly zeros: DESIGN.md §3.11).  Kernels: hificar_feat_kernels.hip.h.
//
// hificar_feat_create touches no device: it checks the configuration and builds the host tables.  The first hificar_feat_forward whose
// arguments pass every check opens the engine and uploads them.

struct hificar_feat {
    hificar_feat_config cfg;
    hificar_engine eng;
    ConvLayer Fdft;
    int nf = 0, nfp = 0, wmax = 0, nc = 0;  // nc: output channels (n_mfcc | num_mels)
    std::vector<int> band;                  // [num_mels][first bin, bins]
    std::vector<float> w;                   // [num_mels][wmax]
    std::vector<float> basis;               // MFCC: [n_mfcc][num_mels]
    int* d_band = nullptr;
    float *d_w = nullptr, *d_basis = nullptr;
    bool ready = false;
    int init_failed = HIFICAR_OK;
};

extern "C" int hificar_feat_create(const hificar_feat_config* cfg, const float* melmat, hificar_feat** out) {
    if (!cfg || !melmat || !out) return fail(HIFICAR_E_INVALID, "hificar_feat_create: null argument");
    const hificar_feat_config& c = *cfg;
    if (c.kind != HIFICAR_FEAT_LOGMEL && c.kind != HIFICAR_FEAT_MFCC) return fail(HIFICAR_E_INVALID, "hificar_feat_create: kind %d", c.kind);
    if (c.fft_size < 32 || c.fft_size % 32 || c.fft_size > 8192 || c.hop_size < 1 || c.win_length < 1 || c.win_length > c.fft_size)
        return fail(HIFICAR_E_INVALID, "hificar_feat_create: fft_size must be a multiple of 32 in 32 .. 8192, 1 <= win_length <= fft_size, hop_size >= 1");
    if (c.num_mels < 1 || c.num_mels > HIFICAR_FEAT_MAX_MELS)
        return fail(HIFICAR_E_INVALID, "hificar_feat_create: num_mels=%d out of range (1 .. %d)", c.num_mels, HIFICAR_FEAT_MAX_MELS);
    if (!(c.amin > 0.f)) return fail(HIFICAR_E_INVALID, "hificar_feat_create: amin / eps must be positive");
    if (c.kind == HIFICAR_FEAT_MFCC && (c.n_mfcc < 1 || c.n_mfcc > c.num_mels))
        return fail(HIFICAR_E_INVALID, "hificar_feat_create: n_mfcc=%d out of range (1 .. num_mels=%d)", c.n_mfcc, c.num_mels);
    if (c.kind == HIFICAR_FEAT_LOGMEL && c.log_base != 0 && c.log_base != 2 && c.log_base != 10)
        return fail(HIFICAR_E_INVALID, "log_base: %d is not supported.", c.log_base);
    hificar_feat* g = new hificar_feat();
    g->cfg = c;
    const int nf = c.fft_size / 2 + 1, nm = c.num_mels;
    g->nf = nf;
    g->nfp = round_up(nf, 32);
    g->nc = c.kind == HIFICAR_FEAT_MFCC ? c.n_mfcc : nm;
    // every band as the run of bins from its first to its last non-zero weight
    g->band.assign((size_t)2 * nm, 0);
    for (int k = 0; k < nm; ++k) {
        int lo = nf, hi = -1;
        for (int f = 0; f < nf; ++f)
            if (melmat[(size_t)k * nf + f] != 0.f) {
                lo = std::min(lo, f);
                hi = f;
            }
        g->band[2 * k] = hi < 0 ? 0 : lo;
        g->band[2 * k + 1] = hi < 0 ? 0 : hi - lo + 1;
        g->wmax = std::max(g->wmax, g->band[2 * k + 1]);
    }
    g->wmax = std::max(g->wmax, 1);
    g->w.assign((size_t)nm * g->wmax, 0.f);
    for (int k = 0; k < nm; ++k)
        for (int j = 0; j < g->band[2 * k + 1]; ++j) g->w[(size_t)k * g->wmax + j] = melmat[(size_t)k * nf + g->band[2 * k] + j];
    if (c.kind == HIFICAR_FEAT_MFCC) {  // scipy.fftpack.dct(type=2, norm="ortho"): formed in double, rounded once
        const double pi = 3.14159265358979323846;
        g->basis.resize((size_t)c.n_mfcc * nm);
        for (int j = 0; j < c.n_mfcc; ++j)
            for (int k = 0; k < nm; ++k)
                g->basis[(size_t)j * nm + k] = (float)(sqrt((j == 0 ? 1.0 : 2.0) / nm) * cos(pi * j * (2 * k + 1) / (2.0 * nm)));
    }
    *out = g;
    return HIFICAR_OK;
}

extern "C" void hificar_feat_destroy(hificar_feat* g) {
    if (!g) return;
    engine_close(&g->eng);  // (opened or not)
    delete g;
}

extern "C" hificar_engine* hificar_feat_engine(hificar_feat* g) { return g ? &g->eng : nullptr; }

extern "C" int hificar_feat_frames(const hificar_feat* g, int L) {
    if (!g || L <= g->cfg.fft_size / 2) return 0;
    return 1 + L / g->cfg.hop_size;
}

struct FeatPlan {
    int Tmax = 0;
    long long M = 0;
    size_t A = 0, S = 0, V = 0, maxv = 0, floats = 0;
};

static bool feat_shape_ok(const hificar_feat* g, int B, int Lmax) {
    if (B < 1 || B > 65535 || Lmax <= g->cfg.fft_size / 2) return false;
    const long long M = (long long)B * (1 + Lmax / g->cfg.hop_size);
    return (M + 256) * std::max(g->cfg.fft_size, 2 * g->nfp) < (1LL << 31);
}

static FeatPlan feat_plan(const hificar_feat* g, int B, int Lmax) {
    FeatPlan p;
    p.Tmax = 1 + Lmax / g->cfg.hop_size;
    p.M = (long long)B * p.Tmax;
    Carver cv(nullptr, 1024);  // (offsets in floats into the caller's workspace)
    const size_t rows = round_up_sz((size_t)p.M, 256);  // whole GEMM tiles of slack behind the last row
    p.A = cv.floats_at(rows * g->cfg.fft_size);
    p.S = cv.floats_at(rows * 2 * g->nfp);
    p.V = cv.floats_at((size_t)p.M * g->cfg.num_mels);
    p.maxv = cv.floats_at((size_t)B);
    p.floats = cv.bytes() / sizeof(float);
    return p;
}

extern "C" size_t hificar_feat_workspace_bytes(const hificar_feat* g, int B, int Lmax) {
    if (!g || !feat_shape_ok(g, B, Lmax)) return 0;
    return feat_plan(g, B, Lmax).floats * sizeof(float);
}

// the engine, the packed DFT matrix and the tables: once per handle, behind the argument checks of the first forward
static int feat_device_init(hificar_feat* g) {
    if (g->init_failed != HIFICAR_OK) return fail(g->init_failed, "hificar_feat: the device state could not be set up on this handle earlier; destroy it");
    hificar_engine* h = &g->eng;
    int rc = engine_open(h, false);
    h->precision = HIFICAR_PREC_F32;
    h->use_pair = false;
    h->ksplit = 0;  // one accumulation order for every launch shape: an utterance's result does not depend on what it is batched with
    auto run = [&]() -> int {
        if (rc != HIFICAR_OK) return rc;
        const int N = g->cfg.fft_size;
        const std::vector<float> dft = mel_dft_matrix(N, g->cfg.win_length, g->nfp);
        if ((rc = mel_make_layer(h, g->Fdft, "feat#dft", N, N, 2 * g->nfp, dft, false, N, 2 * g->nfp)) != HIFICAR_OK) return rc;
        void* p = nullptr;
        HIP_TRY(hipMalloc(&p, g->band.size() * sizeof(int)));
        h->allocs.push_back(p);
        g->d_band = static_cast<int*>(p);
        HIP_TRY(hipMemcpy(g->d_band, g->band.data(), g->band.size() * sizeof(int), hipMemcpyHostToDevice));
        if ((rc = upload(h, g->w, &g->d_w)) != HIFICAR_OK) return rc;
        if (!g->basis.empty() && (rc = upload(h, g->basis, &g->d_basis)) != HIFICAR_OK) return rc;
        HIP_TRY(hipDeviceSynchronize());
        return HIFICAR_OK;
    };
    rc = run();
    if (rc != HIFICAR_OK) return g->init_failed = rc;
    g->ready = true;
    return HIFICAR_OK;
}

extern "C" int hificar_feat_forward(hificar_feat* g, const float* wav, const int32_t* lengths, const int32_t* lengths_host, float* out, int32_t* frames_out,
                                    int B, int Lmax, void* workspace, size_t workspace_bytes, void* stream_) {
    if (!g || !wav || !out) return fail(HIFICAR_E_INVALID, "hificar_feat_forward: null argument");
    const hificar_feat_config& c = g->cfg;
    if (B >= 1 && Lmax <= c.fft_size / 2)
        return fail(HIFICAR_E_INVALID, "hificar_feat_forward: reflect padding needs more than fft_size / 2 = %d samples (Lmax = %d)", c.fft_size / 2, Lmax);
    if (!feat_shape_ok(g, B, Lmax)) return fail(HIFICAR_E_INVALID, "hificar_feat_forward: B=%d, Lmax=%d out of range (B frames fft_size < 2^31)", B, Lmax);
    if (lengths_host && !lengths) return fail(HIFICAR_E_INVALID, "hificar_feat_forward: lengths_host without the device copy");
    if (lengths_host)
        for (int b = 0; b < B; ++b)
            if (lengths_host[b] <= c.fft_size / 2 || lengths_host[b] > Lmax)
                return fail(HIFICAR_E_INVALID, "hificar_feat_forward: lengths[%d]=%d outside fft_size / 2 + 1 = %d .. Lmax=%d", b, lengths_host[b],
                            c.fft_size / 2 + 1, Lmax);
    const FeatPlan p = feat_plan(g, B, Lmax);
    int rc;
    if ((rc = check_workspace(nullptr, workspace, workspace_bytes, p.floats * sizeof(float))) != HIFICAR_OK) return rc;
    // (every argument above is checked without the device)
    if (!g->ready && (rc = feat_device_init(g)) != HIFICAR_OK) return rc;
    hificar_engine* h = &g->eng;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if ((rc = enter_stream(h, stream)) != HIFICAR_OK) return rc;
    float* ws = static_cast<float*>(workspace);
    const int N = c.fft_size, nm = c.num_mels;
    const bool mfcc = c.kind == HIFICAR_FEAT_MFCC;
    {
        FeatFrameParams fp;
        fp.wav = wav;
        fp.lengths = lengths;
        fp.A = ws + p.A;
        fp.total4 = p.M * (N / 4);
        fp.Lmax = Lmax;
        fp.N = N;
        fp.hop = c.hop_size;
        fp.Tmax = p.Tmax;
        ProfScope prof(h, stream, "feat_frame_kernel", 0.0, 8.0 * p.M * N);
        hipLaunchKernelGGL(feat_frame_kernel, dim3(ew_blocks(h, fp.total4)), dim3(256), 0, stream, fp);
        HIP_TRY(hipGetLastError());
    }
    {
        const Ragged rg;
        ConvIO io{};
        io.xs = reinterpret_cast<const char*>(ws + p.A);
        io.y = ws + p.S;
        if ((rc = launch_conv1(h, g->Fdft, 1, (int)p.M, io, 0.f, rg, stream)) != HIFICAR_OK) return rc;
    }
    {
        FeatMelParams mp;
        mp.S = ws + p.S;
        mp.band = g->d_band;
        mp.w = g->d_w;
        mp.V = ws + p.V;
        mp.total = p.M * nm;
        mp.nm = nm;
        mp.nfp = g->nfp;
        mp.wmax = g->wmax;
        mp.amin = c.amin;
        ProfScope prof(h, stream, "feat_mel_kernel", 0.0, 4.0 * p.M * (2.0 * g->nf + nm));
        if (mfcc) hipLaunchKernelGGL(feat_mel_kernel<true>, dim3(ew_blocks(h, mp.total)), dim3(256), 0, stream, mp);
        else hipLaunchKernelGGL(feat_mel_kernel<false>, dim3(ew_blocks(h, mp.total)), dim3(256), 0, stream, mp);
        HIP_TRY(hipGetLastError());
    }
    if (mfcc && c.top_db >= 0.f) {
        ProfScope prof(h, stream, "feat_db_max_kernel", 0.0, 4.0 * p.M * nm);
        hipLaunchKernelGGL(feat_db_max_kernel, dim3((unsigned)B), dim3(256), 0, stream, ws + p.V, lengths, ws + p.maxv, nm, Lmax, N, c.hop_size, p.Tmax);
        HIP_TRY(hipGetLastError());
    }
    FeatOutParams op;
    memset(&op, 0, sizeof(op));
    op.V = ws + p.V;
    op.lengths = lengths;
    op.maxv = ws + p.maxv;
    op.basis = g->d_basis;
    op.out = out;
    op.frames_out = frames_out;
    op.nm = nm;
    op.nc = g->nc;
    op.Lmax = Lmax;
    op.N = N;
    op.hop = c.hop_size;
    op.Tmax = p.Tmax;
    op.top_db = c.top_db;
    op.eps = c.amin;
    op.log_base = c.log_base;
    const dim3 grid((unsigned)((p.Tmax + 31) / 32), (unsigned)B);
    ProfScope prof(h, stream, mfcc ? "feat_mfcc_out_kernel" : "feat_logmel_out_kernel", 0.0, 4.0 * p.M * (nm + g->nc));
    if (mfcc) hipLaunchKernelGGL(feat_mfcc_out_kernel, grid, dim3(256), 0, stream, op);
    else hipLaunchKernelGGL(feat_logmel_out_kernel, grid, dim3(256), 0, stream, op);
    HIP_TRY(hipGetLastError());
    return HIFICAR_OK;
}
