// A linear head on device features: y[b, :, t] = W x[b, :, t] + bias over (B, in, T) -> (B, out, T), the fitted linear regression the
// reference's egs/ema/voc1/local/linear_inference.py applies to WavLM's hidden states.  The one-tap GEMM every Linear of this library is:
//   rows   (B, in, T) -> channels-last rows [B T][in_pad]                 xfmr_rows_kernel
//   GEMM   rows x W^T + bias under the ragged context                     conv engine (exact fp32, split-K off)
//   out    rows -> (B, out, T), exact zeros from an utterance's length on     xfmr_out_kernel
// Every utterance is computed as if alone, bit for bit.

struct hificar_linear {
    hificar_engine eng;
    ConvLayer w;
    int in = 0, out = 0, in_pad = 0;
};

extern "C" int hificar_linear_create(int in_features, int out_features, const float* coef, const float* intercept, hificar_linear** out) {
    if (!coef || !intercept || !out) return fail(HIFICAR_E_INVALID, "hificar_linear_create: null argument");
    if (in_features < 1 || in_features > HIFICAR_LINEAR_MAX_IN || out_features < 1 || out_features > HIFICAR_LINEAR_MAX_OUT)
        return fail(HIFICAR_E_INVALID, "LinearHead: %d -> %d features out of range (1 .. %d in, 1 .. %d out)", in_features, out_features,
                    HIFICAR_LINEAR_MAX_IN, HIFICAR_LINEAR_MAX_OUT);
    hificar_linear* g = new hificar_linear();
    g->in = in_features;
    g->out = out_features;
    g->in_pad = round_up(in_features, 32);
    int rc = xfmr_plan(g->w, "linear_head", in_features, g->in_pad, out_features, 1);
    hificar_engine* h = &g->eng;
    h->precision = HIFICAR_PREC_F32;
    if (rc == HIFICAR_OK) {
        HostTensor W;
        W.shape = {out_features, in_features, 1};
        W.data.assign(coef, coef + (size_t)out_features * in_features);
        const std::vector<float> bias(intercept, intercept + out_features);
        rc = xfmr_pack(h, g->w, W, &bias);
    }
    if (rc == HIFICAR_OK) rc = engine_open(h, true);
    if (rc != HIFICAR_OK) {
        engine_close(h);
        delete g;
        return rc;
    }
    h->precision = HIFICAR_PREC_F32;
    h->use_pair = false;
    h->ksplit = 0;  // one accumulation order for every launch shape
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        engine_close(h);
        delete g;
        return fail(HIFICAR_E_HIP, "hificar_linear_create: %s", hipGetErrorString(e));
    }
    *out = g;
    return HIFICAR_OK;
}

extern "C" void hificar_linear_destroy(hificar_linear* g) {
    if (!g) return;
    engine_close(&g->eng);
    delete g;
}

extern "C" hificar_engine* hificar_linear_engine(hificar_linear* g) { return g ? &g->eng : nullptr; }

static bool linear_shape_ok(const hificar_linear* g, int B, int T) {
    return g && B >= 1 && B <= 65535 && T >= 1 && (long long)B * T * std::max(g->in_pad, g->w.cout_pad) < (1LL << 31);
}

struct LinearWorkspace {
    float* xin;  // [rows][in_pad]
    float* y;    // [rows][cout_pad]
    size_t bytes;
};

static LinearWorkspace linear_plan_workspace(const hificar_linear* g, int B, int T, void* base) {
    const size_t rows = round_up_sz((size_t)B * (size_t)T, 256);  // whole tiles of slack behind the last row
    LinearWorkspace w;
    Carver cv(base, 256);
    w.xin = cv.floats(rows * g->in_pad);
    w.y = cv.floats(rows * g->w.cout_pad);
    w.bytes = cv.bytes();
    return w;
}

extern "C" size_t hificar_linear_workspace_bytes(const hificar_linear* g, int B, int T) {
    if (!linear_shape_ok(g, B, T)) return 0;
    return linear_plan_workspace(g, B, T, nullptr).bytes;
}

extern "C" int hificar_linear_forward(hificar_linear* g, const float* x, const int32_t* lengths, float* out, int B, int T, void* workspace,
                                      size_t workspace_bytes, void* stream_) {
    if (!g || !x || !out) return fail(HIFICAR_E_INVALID, "hificar_linear_forward: null argument");
    if (!linear_shape_ok(g, B, T)) return fail(HIFICAR_E_INVALID, "hificar_linear_forward: B=%d, T=%d out of range (B <= 65535, B T max(in, out) < 2^31)", B, T);
    const LinearWorkspace ws = linear_plan_workspace(g, B, T, workspace);
    int rc;
    if ((rc = check_workspace(nullptr, workspace, workspace_bytes, ws.bytes)) != HIFICAR_OK) return rc;
    hificar_engine* h = &g->eng;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if ((rc = enter_stream(h, stream)) != HIFICAR_OK) return rc;
    float* const xin = ws.xin;
    float* const y = ws.y;
    const double M = (double)B * T;
    const int Op = g->w.cout_pad;
    {
        ProfScope prof(h, stream, "xfmr_rows_kernel", 0.0, 4.0 * M * (g->in + g->in_pad));
        hipLaunchKernelGGL(xfmr_rows_kernel, dim3((unsigned)((T + 31) / 32), (unsigned)(g->in_pad / 32), (unsigned)B), dim3(256), 0, stream, x, xin,
                           static_cast<const int*>(lengths), g->in, g->in_pad, T, static_cast<const int*>(nullptr));
        HIP_TRY(hipGetLastError());
    }
    Ragged rg;
    rg.seq_len = lengths;
    rg.frames = T;
    ConvIO io{};
    io.xs = reinterpret_cast<const char*>(xin);
    io.res = nullptr;
    io.y = y;
    io.ys = nullptr;
    if ((rc = launch_conv1(h, g->w, B, T, io, 0.f, rg, stream)) != HIFICAR_OK) return rc;
    {
        ProfScope prof(h, stream, "xfmr_out_kernel", 0.0, 4.0 * M * (g->out + Op));
        hipLaunchKernelGGL(xfmr_out_kernel, dim3((unsigned)((T + 31) / 32), (unsigned)(Op / 32), (unsigned)B), dim3(256), 0, stream, static_cast<const float*>(y),
                           out, static_cast<const int*>(lengths), g->out, Op, T, static_cast<const int*>(nullptr));
        HIP_TRY(hipGetLastError());
    }
    return HIFICAR_OK;
}
