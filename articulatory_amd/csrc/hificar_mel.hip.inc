// Mel-spectrogram loss of the train step (articulatory/losses/mel_loss.py:114-166, called at articulatory/bin/train.py:308-311): value and
// gradient with respect to the generated waveform in one call.  STFT = frame gather + one GEMM against the windowed DFT matrix, mel =
// one GEMM against the filterbank, both on the exact-fp32 conv kernels; backward = the transposed GEMMs + overlap-add.

struct hificar_mel {
    hificar_mel_config cfg;
    hificar_engine eng;
    ConvLayer Fdft, Ddft, Fmel, Dmel;
    int nf = 0, nfp = 0, mp = 0;
};

static int mel_make_layer(hificar_engine* h, ConvLayer& L, const char* name, int cin, int cin_pad, int cout, const std::vector<float>& w_ref /* (cout, cin) */,
                          bool transpose_src, int src_cin, int src_cout) {
    L = ConvLayer();
    L.name = name;
    L.cin = cin;
    L.cin_pad = cin_pad;
    L.cout = cout;
    L.K = 1;
    L.dilation = 1;
    L.padding = 0;
    L.has_bias = false;
    int rc = plan_layer(L);
    if (rc != HIFICAR_OK) return rc;
    void* p = nullptr;
    const size_t pe = pack_w32_elems(L, L.chunk16);
    HIP_TRY(hipMalloc(&p, pe * sizeof(float)));
    h->allocs.push_back(p);
    HIP_TRY(hipMemset(p, 0, pe * sizeof(float)));
    L.d_w32 = static_cast<float*>(p);
    HIP_TRY(hipMalloc(&p, (size_t)L.cout_total * sizeof(float)));
    h->allocs.push_back(p);
    HIP_TRY(hipMemset(p, 0, (size_t)L.cout_total * sizeof(float)));
    L.d_bias = static_cast<float*>(p);
    float* d_src = nullptr;
    if ((rc = upload(h, w_ref, &d_src)) != HIFICAR_OK) return rc;
    PackParams pp;
    fill_pack(pp, L, L.chunk16);
    pp.src = d_src;
    pp.dst = L.d_w32;
    pp.mode = transpose_src ? 2 : 0;  // 2: w'[co'][ci'] = W[ci'][co'] of the (src_cout, src_cin) matrix
    pp.cin = src_cin;
    pp.cout = src_cout;
    pp.K = 1;
    pp.cin_pack = cin;
    pp.cout_pack = cout;
    return launch_pack(pp, nullptr);
}

// windowed DFT matrix (2 nfp, N): rows [0, nf) = w[n] cos(2 pi f n / N), rows [nfp, nfp + nf) = -w[n] sin(...); torch.hann_window is
// periodic, a shorter window sits centred in the frame (torch.stft, librosa.stft)
static std::vector<float> mel_dft_matrix(int N, int win_length, int nfp) {
    const int nf = N / 2 + 1;
    std::vector<float> dft((size_t)2 * nfp * N, 0.f);
    const int w0 = (N - win_length) / 2;
    const double pi = 3.14159265358979323846;
    for (int n = 0; n < N; ++n) {
        const int wn = n - w0;
        const double w = (wn >= 0 && wn < win_length) ? 0.5 - 0.5 * cos(2.0 * pi * wn / win_length) : 0.0;
        for (int f = 0; f < nf; ++f) {
            const double ang = 2.0 * pi * (double)(((long long)f * n) % N) / N;
            dft[(size_t)f * N + n] = (float)(w * cos(ang));
            dft[(size_t)(nfp + f) * N + n] = (float)(-w * sin(ang));
        }
    }
    return dft;
}

extern "C" int hificar_mel_create(const hificar_mel_config* cfg, const float* melmat, hificar_mel** out) {
    if (!cfg || !out || (!melmat && cfg->mode == 0)) return fail(HIFICAR_E_INVALID, "hificar_mel_create: null argument");
    const hificar_mel_config& c = *cfg;
    if (c.mode != 0 && c.mode != 1) return fail(HIFICAR_E_INVALID, "mel / STFT loss: mode %d", c.mode);
    if (c.fft_size < 32 || c.fft_size % 32 || c.hop_size < 1 || c.win_length < 1 || c.win_length > c.fft_size || (c.mode == 0 && c.num_mels < 1) ||
        !(c.eps > 0.f))
        return fail(HIFICAR_E_INVALID, "mel loss: fft_size must be a multiple of 32, 1 <= win_length <= fft_size, hop_size / num_mels >= 1, eps > 0");
    if (c.log_base != 0 && c.log_base != 2 && c.log_base != 10) return fail(HIFICAR_E_INVALID, "log_base: %d is not supported.", c.log_base);
    hificar_mel* m = new hificar_mel();
    m->cfg = c;
    hificar_engine* h = &m->eng;
    int rc = engine_open(h, false);  // (this engine has never read the environment switches: inherited behaviour, not a decision)
    h->precision = HIFICAR_PREC_F32;
    h->use_pair = false;
    auto bail = [&](int code) {
        engine_close(h);
        delete m;
        return code;
    };
    if (rc != HIFICAR_OK) return bail(rc);
    const int N = c.fft_size, nf = N / 2 + 1, nfp = round_up(nf, 32), mp = round_up(std::max(c.num_mels, 1), 32);
    m->nf = nf;
    m->nfp = nfp;
    m->mp = mp;
    const std::vector<float> dft = mel_dft_matrix(N, c.win_length, nfp);
    if ((rc = mel_make_layer(h, m->Fdft, "mel#dft", N, N, 2 * nfp, dft, false, N, 2 * nfp)) != HIFICAR_OK) return bail(rc);
    if ((rc = mel_make_layer(h, m->Ddft, "mel#dft^T", 2 * nfp, 2 * nfp, N, dft, true, N, 2 * nfp)) != HIFICAR_OK) return bail(rc);
    if (c.mode == 0) {
        std::vector<float> mel((size_t)c.num_mels * nfp, 0.f);  // (num_mels, nfp)
        for (int k = 0; k < c.num_mels; ++k)
            for (int f = 0; f < nf; ++f) mel[(size_t)k * nfp + f] = melmat[(size_t)k * nf + f];
        if ((rc = mel_make_layer(h, m->Fmel, "mel#fb", nfp, nfp, c.num_mels, mel, false, nfp, c.num_mels)) != HIFICAR_OK) return bail(rc);
        if ((rc = mel_make_layer(h, m->Dmel, "mel#fb^T", c.num_mels, mp, nfp, mel, true, nfp, c.num_mels)) != HIFICAR_OK) return bail(rc);
    }
    HIP_TRY(hipDeviceSynchronize());
    *out = m;
    return HIFICAR_OK;
}

extern "C" void hificar_mel_destroy(hificar_mel* m) {
    if (!m) return;
    engine_close(&m->eng);
    delete m;
}

struct MelPlan {
    int frames = 0;
    long long M = 0;
    size_t A[2], S[2], amp[2], mel[2];  // [0] generated, [1] ground truth
    size_t dmel = 0, damp = 0, dS = 0, dA = 0, partial = 0;
    size_t floats = 0;
};

static constexpr int kMelLossBlocks = 64;

static MelPlan mel_plan(const hificar_mel* m, int B, int T) {
    MelPlan p;
    p.frames = 1 + T / m->cfg.hop_size;
    p.M = (long long)B * p.frames;
    Carver cv(nullptr, 1024);  // (offsets in floats into the caller's workspace)
    const size_t M = (size_t)p.M, N = (size_t)m->cfg.fft_size;
    for (int i = 0; i < 2; ++i) {
        p.A[i] = cv.floats_at(M * N);
        p.S[i] = cv.floats_at(M * 2 * m->nfp);
        p.amp[i] = cv.floats_at(M * m->nfp);
        p.mel[i] = cv.floats_at(M * m->mp);
    }
    p.dmel = cv.floats_at(M * m->mp);
    p.damp = cv.floats_at(M * m->nfp);
    p.dS = cv.floats_at(M * 2 * m->nfp);
    p.dA = cv.floats_at(M * N);
    p.partial = cv.floats_at(kMelLossBlocks * 3 + 8);  // (STFT mode: [blocks][3] partials, then the 4 totals)
    p.floats = cv.bytes() / sizeof(float);
    return p;
}

extern "C" size_t hificar_mel_workspace_bytes(const hificar_mel* m, int B, int T) {
    if (!m || B < 1 || T < 1) return 0;
    return mel_plan(m, B, T).floats * sizeof(float);
}

// value[0] = MelSpectrogramLoss(y_hat, y) (device float); dy_hat (B, T) = its gradient with respect to y_hat, or NULL.
extern "C" int hificar_mel_loss(hificar_mel* m, const float* y_hat, const float* y, int B, int T, float* value, float* dy_hat, void* ws_, size_t ws_bytes,
                                void* stream_) {
    if (!m || !y_hat || !y || !value || !ws_) return fail(HIFICAR_E_INVALID, "hificar_mel_loss: null argument");
    const hificar_mel_config& c = m->cfg;
    if (c.mode != 0) return fail(HIFICAR_E_STATE, "hificar_mel_loss on an STFT-loss handle (use hificar_stft_loss_forward / _backward)");
    if (B < 1 || T <= c.fft_size / 2) return fail(HIFICAR_E_INVALID, "mel loss: reflect padding needs T > fft_size / 2 (T = %d)", T);
    const MelPlan p = mel_plan(m, B, T);
    if (ws_bytes < p.floats * sizeof(float)) return fail(HIFICAR_E_WORKSPACE, "mel loss workspace too small");
    if (reinterpret_cast<uintptr_t>(ws_) % 256) return fail(HIFICAR_E_INVALID, "mel loss workspace must be 256-byte aligned");
    hificar_engine* h = &m->eng;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    int rc;
    if ((rc = enter_stream(h, stream)) != HIFICAR_OK) return rc;
    float* ws = static_cast<float*>(ws_);
    const Ragged rg;
    const int N = c.fft_size;
    auto gemm = [&](const ConvLayer& L, const float* x, float* y_out) {
        ConvIO io{};
        io.xs = reinterpret_cast<const char*>(x);
        io.y = y_out;
        return launch_conv1(h, L, 1, (int)p.M, io, 0.f, rg, stream);
    };
    for (int i = 0; i < 2; ++i) {
        FrameParams fp;
        fp.y = i == 0 ? y_hat : y;
        fp.A = ws + p.A[i];
        fp.total4 = p.M * (N / 4);
        fp.T = T;
        fp.N = N;
        fp.hop = c.hop_size;
        fp.frames = p.frames;
        hipLaunchKernelGGL(mel_frame_kernel, dim3(ew_blocks(h, fp.total4)), dim3(256), 0, stream, fp);
        HIP_TRY(hipGetLastError());
        if ((rc = gemm(m->Fdft, ws + p.A[i], ws + p.S[i])) != HIFICAR_OK) return rc;
        AmpParams ap;
        memset(&ap, 0, sizeof(ap));
        ap.S = ws + p.S[i];
        ap.amp = ws + p.amp[i];
        ap.total = p.M * m->nfp;
        ap.nf = m->nf;
        ap.nfp = m->nfp;
        ap.eps = c.eps;
        hipLaunchKernelGGL(mel_amp_kernel, dim3(ew_blocks(h, ap.total)), dim3(256), 0, stream, ap);
        HIP_TRY(hipGetLastError());
        if ((rc = gemm(m->Fmel, ws + p.amp[i], ws + p.mel[i])) != HIFICAR_OK) return rc;
    }
    MelLossParams lp;
    lp.mel_hat = ws + p.mel[0];
    lp.mel = ws + p.mel[1];
    lp.dmel_hat = dy_hat ? ws + p.dmel : nullptr;
    lp.partial = ws + p.partial;
    lp.total = p.M * m->mp;
    lp.nm = c.num_mels;
    lp.mp = m->mp;
    lp.eps = c.eps;
    lp.log_scale = c.log_base == 0 ? 1.f : (float)(1.0 / log((double)c.log_base));
    lp.inv_numel = (float)(1.0 / ((double)p.M * c.num_mels));
    hipLaunchKernelGGL(mel_loss_kernel, dim3(kMelLossBlocks), dim3(256), 0, stream, lp);
    HIP_TRY(hipGetLastError());
    VreduceParams vp;
    memset(&vp, 0, sizeof(vp));
    vp.partial = ws + p.partial;
    vp.n = kMelLossBlocks;
    vp.stride = 1;
    vp.len = 1;
    vp.dst = value;
    hipLaunchKernelGGL(vreduce_kernel, dim3(1), dim3(256), 0, stream, vp);
    HIP_TRY(hipGetLastError());
    if (!dy_hat) return HIFICAR_OK;
    if ((rc = gemm(m->Dmel, ws + p.dmel, ws + p.damp)) != HIFICAR_OK) return rc;
    AmpParams ap;
    memset(&ap, 0, sizeof(ap));
    ap.S = ws + p.S[0];
    ap.damp = ws + p.damp;
    ap.dS = ws + p.dS;
    ap.total = p.M * m->nfp;
    ap.nf = m->nf;
    ap.nfp = m->nfp;
    ap.eps = c.eps;
    hipLaunchKernelGGL(mel_amp_bwd_kernel, dim3(ew_blocks(h, ap.total)), dim3(256), 0, stream, ap);
    HIP_TRY(hipGetLastError());
    if ((rc = gemm(m->Ddft, ws + p.dS, ws + p.dA)) != HIFICAR_OK) return rc;
    OlaParams op;
    op.dA = ws + p.dA;
    op.dy = dy_hat;
    op.total = (long long)B * T;
    op.T = T;
    op.N = N;
    op.hop = c.hop_size;
    op.frames = p.frames;
    hipLaunchKernelGGL(mel_ola_kernel, dim3(ew_blocks(h, op.total)), dim3(256), 0, stream, op);
    HIP_TRY(hipGetLastError());
    return HIFICAR_OK;
}

// ------------------------------------------------------------------------------------------------
// One resolution of MultiResolutionSTFTLoss (stft_loss.py:87-125) on a handle created with mode = 1: forward leaves the magnitudes in the
// workspace, backward takes the upstream gradients of (sc, mag) from device memory (no host synchronisation).
// ------------------------------------------------------------------------------------------------
static void stft_params(const hificar_mel* m, const MelPlan& p, float* ws, StftLossParams& lp) {
    memset(&lp, 0, sizeof(lp));
    lp.x = ws + p.amp[0];
    lp.y = ws + p.amp[1];
    lp.partial = ws + p.partial;
    lp.sums = ws + p.partial + kMelLossBlocks * 3;
    lp.total = p.M * m->nfp;
    lp.nf = m->nf;
    lp.nfp = m->nfp;
    lp.blocks = kMelLossBlocks;
    lp.inv_numel = (float)(1.0 / ((double)p.M * m->nf));
}

extern "C" int hificar_stft_loss_forward(hificar_mel* m, const float* y_hat, const float* y, int B, int T, float* values2, void* ws_, size_t ws_bytes,
                                         void* stream_) {
    if (!m || !y_hat || !y || !values2 || !ws_) return fail(HIFICAR_E_INVALID, "hificar_stft_loss_forward: null argument");
    const hificar_mel_config& c = m->cfg;
    if (c.mode != 1) return fail(HIFICAR_E_STATE, "hificar_stft_loss_forward needs a handle created with mode = 1");
    if (B < 1 || T <= c.fft_size / 2) return fail(HIFICAR_E_INVALID, "STFT loss: reflect padding needs T > fft_size / 2 (T = %d)", T);
    const MelPlan p = mel_plan(m, B, T);
    if (ws_bytes < p.floats * sizeof(float)) return fail(HIFICAR_E_WORKSPACE, "STFT loss workspace too small");
    if (reinterpret_cast<uintptr_t>(ws_) % 256) return fail(HIFICAR_E_INVALID, "STFT loss workspace must be 256-byte aligned");
    hificar_engine* h = &m->eng;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    int rc;
    if ((rc = enter_stream(h, stream)) != HIFICAR_OK) return rc;
    float* ws = static_cast<float*>(ws_);
    const Ragged rg;
    const int N = c.fft_size;
    for (int i = 0; i < 2; ++i) {
        FrameParams fp;
        fp.y = i == 0 ? y_hat : y;
        fp.A = ws + p.A[i];
        fp.total4 = p.M * (N / 4);
        fp.T = T;
        fp.N = N;
        fp.hop = c.hop_size;
        fp.frames = p.frames;
        hipLaunchKernelGGL(mel_frame_kernel, dim3(ew_blocks(h, fp.total4)), dim3(256), 0, stream, fp);
        HIP_TRY(hipGetLastError());
        ConvIO io{};
        io.xs = reinterpret_cast<const char*>(ws + p.A[i]);
        io.y = ws + p.S[i];
        if ((rc = launch_conv1(h, m->Fdft, 1, (int)p.M, io, 0.f, rg, stream)) != HIFICAR_OK) return rc;
        AmpParams ap;
        memset(&ap, 0, sizeof(ap));
        ap.S = ws + p.S[i];
        ap.amp = ws + p.amp[i];
        ap.total = p.M * m->nfp;
        ap.nf = m->nf;
        ap.nfp = m->nfp;
        ap.eps = c.eps;
        hipLaunchKernelGGL(mel_amp_kernel, dim3(ew_blocks(h, ap.total)), dim3(256), 0, stream, ap);
        HIP_TRY(hipGetLastError());
    }
    StftLossParams lp;
    stft_params(m, p, ws, lp);
    lp.values = values2;
    hipLaunchKernelGGL(stft_loss_sums_kernel, dim3(kMelLossBlocks), dim3(256), 0, stream, lp);
    hipLaunchKernelGGL(stft_loss_final_kernel, dim3(1), dim3(64), 0, stream, lp);
    HIP_TRY(hipGetLastError());
    return HIFICAR_OK;
}

// dy_hat (B, T) = d(gweights[0] * sc + gweights[1] * mag) / dy_hat of the forward whose workspace this is.
extern "C" int hificar_stft_loss_backward(hificar_mel* m, int B, int T, const float* gweights2, float* dy_hat, void* ws_, size_t ws_bytes, void* stream_) {
    if (!m || !gweights2 || !dy_hat || !ws_) return fail(HIFICAR_E_INVALID, "hificar_stft_loss_backward: null argument");
    const hificar_mel_config& c = m->cfg;
    if (c.mode != 1) return fail(HIFICAR_E_STATE, "hificar_stft_loss_backward needs a handle created with mode = 1");
    const MelPlan p = mel_plan(m, B, T);
    if (ws_bytes < p.floats * sizeof(float)) return fail(HIFICAR_E_WORKSPACE, "STFT loss workspace too small");
    hificar_engine* h = &m->eng;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    int rc;
    if ((rc = enter_stream(h, stream)) != HIFICAR_OK) return rc;
    float* ws = static_cast<float*>(ws_);
    const Ragged rg;
    StftLossParams lp;
    stft_params(m, p, ws, lp);
    lp.gw = gweights2;
    lp.dx = ws + p.damp;
    hipLaunchKernelGGL(stft_loss_grad_kernel, dim3(ew_blocks(h, lp.total)), dim3(256), 0, stream, lp);
    HIP_TRY(hipGetLastError());
    AmpParams ap;
    memset(&ap, 0, sizeof(ap));
    ap.S = ws + p.S[0];
    ap.damp = ws + p.damp;
    ap.dS = ws + p.dS;
    ap.total = p.M * m->nfp;
    ap.nf = m->nf;
    ap.nfp = m->nfp;
    ap.eps = c.eps;
    hipLaunchKernelGGL(mel_amp_bwd_kernel, dim3(ew_blocks(h, ap.total)), dim3(256), 0, stream, ap);
    HIP_TRY(hipGetLastError());
    ConvIO io{};
    io.xs = reinterpret_cast<const char*>(ws + p.dS);
    io.y = ws + p.dA;
    if ((rc = launch_conv1(h, m->Ddft, 1, (int)p.M, io, 0.f, rg, stream)) != HIFICAR_OK) return rc;
    OlaParams op;
    op.dA = ws + p.dA;
    op.dy = dy_hat;
    op.total = (long long)B * T;
    op.T = T;
    op.N = c.fft_size;
    op.hop = c.hop_size;
    op.frames = p.frames;
    hipLaunchKernelGGL(mel_ola_kernel, dim3(ew_blocks(h, op.total)), dim3(256), 0, stream, op);
    HIP_TRY(hipGetLastError());
    return HIFICAR_OK;
}
