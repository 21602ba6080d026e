// GBlockGenerator on the conv engine (included by hificar.hip behind hificar_train.hip.inc).  Reference: articulatory/models/gblock_gen.py:14-132
// (the generator), articulatory/layers/pytorch_layers.py:32-91 (GBlock).  SURVEY.md §8 f4.
//
//   c = input_conv(cat(c, PastFCEncoder(ar)) [+ spk])                    front_kernel + one conv launch (raw rows + ReLU'd rows)
//   per GBlock (scale s, kernel k):                                       FOUR conv launches, nothing else:
//     h1 = conv_k(up_s(ReLU(x)))       r = conv_1(up_s(x))                1. two branches of ONE launch over the same input rows; the nearest
//                                                                            upsample is a row map in the LDS staging (ConvParams::x_up): the
//                                                                            upsampled tensor never exists; r is the one true pointwise GEMM
//     y  = conv_k,d3(ReLU(h1)) + r                                         2. residual epilogue (res = r), writes y and ReLU(y)
//     h3 = conv_k,d9(ReLU(y))                                              3.
//     out = y + conv_k,d27(ReLU(h3))                                       4. residual epilogue (res = y), writes out and ReLU(out)
//   wave = tanh(conv(LeakyReLU_0.01(out)))                                 output_conv_kernel
// ReLU is LeakyReLU with slope 0 in the output pass.  Exact fp32 only: r contracts over the RAW rows, which in the bf16x3 arithmetic would
// need a second split copy of every block output.

static const int kGblockIn[HIFICAR_MAX_GBLOCKS] = {1, 1, 1, 2, 2, 2, 2, 4, 4, 8};   // gblock_gen.py:63
static const int kGblockOut[HIFICAR_MAX_GBLOCKS] = {1, 1, 2, 2, 2, 2, 4, 4, 8, 8};  // gblock_gen.py:64

extern "C" int hificar_gblock_create(const hificar_gblock_config* gc, hificar_handle** out) {
    if (!gc || !out) return fail(HIFICAR_E_INVALID, "hificar_gblock_create: null argument");
    const hificar_gblock_config& c = *gc;
    if (c.out_channels != 1) return fail(HIFICAR_E_INVALID, "out_channels=%d unsupported", c.out_channels);
    if (c.kernel_size % 2 != 1) return fail(HIFICAR_E_INVALID, "Kernel size must be odd number.");
    if (c.kernel_size > kMaxTaps) return fail(HIFICAR_E_INVALID, "kernel_size=%d > %d", c.kernel_size, kMaxTaps);
    if (c.n_blocks < 1 || c.n_blocks > HIFICAR_MAX_GBLOCKS)
        return fail(HIFICAR_E_INVALID, "%d GBlocks: the reference's channel plan has %d entries (gblock_gen.py:63-64)", c.n_blocks, HIFICAR_MAX_GBLOCKS);
    if (c.channels / 8 < 1) return fail(HIFICAR_E_INVALID, "channels=%d leaves no channels for the last GBlocks", c.channels);
    if (c.channels / kGblockOut[c.n_blocks - 1] != c.channels / 8)
        return fail(HIFICAR_E_INVALID, "%d GBlocks end at channels // %d channels but the output conv takes channels // 8 (gblock_gen.py:63-64, 75-76): "
                    "the reference class only runs with 9 or 10 GBlocks", c.n_blocks, kGblockOut[c.n_blocks - 1]);
    for (int i = 0; i < c.n_blocks; ++i) {
        if (c.g_kernel_sizes[i] % 2 != 1)
            return fail(HIFICAR_E_INVALID, "g_kernel_sizes[%d]=%d: a GBlock with an even kernel loses samples against its residual path in the reference "
                        "(pytorch_layers.py:24-29, 85-91); odd sizes only", i, c.g_kernel_sizes[i]);
        // the dilation-27 conv reaches 13.5 (k - 1) rows either side: at k = 11 a 32-row tile with its 270-row halo is 77 KB per staging buffer at
        // 64-channel chunks — the last size two buffers of which fit the 160-KB LDS (the tile picker skips every taller shape by itself)
        if (c.g_kernel_sizes[i] > 11) return fail(HIFICAR_E_INVALID, "g_kernel_sizes[%d]=%d > 11 (the dilation-27 conv's halo must fit the LDS tiles)", i, c.g_kernel_sizes[i]);
        if (c.g_scales[i] < 1 || c.g_scales[i] > 64) return fail(HIFICAR_E_INVALID, "g_scales[%d]=%d out of range", i, c.g_scales[i]);
    }
    if (c.use_ar && (c.ar_input > 1024 || c.ar_hidden > 512 || c.ar_output > 512 || c.ar_input < 1))
        return fail(HIFICAR_E_INVALID, "PastFCEncoder: ar_input must be <= 1024, ar_hidden / ar_output <= 512");
    if (c.use_ar && (c.ar_hidden % 4 != 0 || c.ar_output % 4 != 0))
        return fail(HIFICAR_E_INVALID, "PastFCEncoder hidden/output dims must be multiples of 4");
    if (c.precision != HIFICAR_PREC_F32)
        return fail(HIFICAR_E_INVALID, "GBlockGenerator runs in the exact-fp32 arithmetic only (its 1 x 1 residual conv reads raw, un-activated rows)");
    if (c.use_spk_id && (c.num_spk < 1 || c.spk_emb_size < 1 || c.in_channels > 1024))
        return fail(HIFICAR_E_INVALID, "use_spk_id needs num_spk and spk_emb_size (and in_channels <= 1024)");

    hificar_handle* h = new hificar_handle();
    h->arch = 1;
    hificar_config& g = h->cfg;
    memset(&g, 0, sizeof(g));
    g.in_channels = c.in_channels;
    g.out_channels = c.out_channels;
    g.channels = c.channels;
    g.kernel_size = c.kernel_size;
    g.n_stages = 0;
    g.n_blocks = 1;
    g.use_additional_convs = 1;
    g.bias = 1;
    g.lrelu_slope = 0.f;  // ReLU
    g.use_tanh = c.use_tanh;
    g.use_ar = c.use_ar;
    g.ar_input = c.ar_input;
    g.ar_hidden = c.ar_hidden;
    g.ar_output = c.ar_output;
    g.precision = HIFICAR_PREC_F32;
    g.use_spk_id = c.use_spk_id;
    g.num_spk = c.num_spk;
    g.spk_emb_size = c.spk_emb_size;
    h->precision = HIFICAR_PREC_F32;
    h->cf = c.in_channels - (c.use_ar ? c.ar_output : 0);
    if (h->cf < 1) {
        delete h;
        return fail(HIFICAR_E_INVALID, "in_channels=%d leaves no feature channels", c.in_channels);
    }
    h->cin_pad = std::max(32, round_up(c.in_channels, 16));
    h->hop = 1;
    for (int i = 0; i < c.n_blocks; ++i) h->hop *= c.g_scales[i];
    h->c_last = c.channels / 8;

    int rc = HIFICAR_OK;
    auto expect = [&](const std::string& n, std::vector<int64_t> s) { h->weights.expected[n] = s; };
    ConvLayer& ic = h->input_conv;
    ic.name = "input_conv";
    ic.cin = c.in_channels;
    ic.cin_pad = h->cin_pad;
    ic.cout = c.channels;
    ic.K = c.kernel_size;
    ic.padding = (c.kernel_size - 1) / 2;
    rc = plan_layer(ic);
    expect("input_conv.weight", {c.channels, c.in_channels, c.kernel_size});
    expect("input_conv.bias", {c.channels});
    h->gb.resize((size_t)c.n_blocks);
    for (int i = 0; i < c.n_blocks && rc == HIFICAR_OK; ++i) {
        GBlockLayers& b = h->gb[(size_t)i];
        b.scale = c.g_scales[i];
        b.cin = c.channels / kGblockIn[i];
        b.cout = c.channels / kGblockOut[i];
        const int k = c.g_kernel_sizes[i], u = b.scale > 1 ? 1 : 0;  // an Upsample module moves the Sequentials' conv indices by one
        const std::string base = "resamples." + std::to_string(i);
        struct Spec {
            ConvLayer* L;
            std::string name;
            int cin, K, dil;
        } specs[5] = {{&b.c1a, base + ".conv1." + std::to_string(1 + u), b.cin, k, 1},
                      {&b.c1b, base + ".conv1." + std::to_string(3 + u), b.cout, k, 3},
                      {&b.res, base + ".res1." + std::to_string(u), b.cin, 1, 1},
                      {&b.c2a, base + ".conv2.1", b.cout, k, 9},
                      {&b.c2b, base + ".conv2.3", b.cout, k, 27}};
        for (const Spec& sp : specs) {
            ConvLayer& L = *sp.L;
            L.name = sp.name;
            L.cin = sp.cin;
            L.cin_pad = round_up(sp.cin, 32);
            L.cout = b.cout;
            L.K = sp.K;
            L.dilation = sp.dil;
            L.padding = sp.dil * (sp.K - 1) / 2;  // get_padding, pytorch_layers.py:24-29
            if ((rc = plan_layer(L)) != HIFICAR_OK) break;
            expect(L.name + ".weight", {L.cout, L.cin, L.K});
            expect(L.name + ".bias", {L.cout});
        }
    }
    expect("output_conv.1.weight", {1, h->c_last, c.kernel_size});
    expect("output_conv.1.bias", {1});
    if (c.use_ar) {
        int dims[6] = {c.ar_input, c.ar_hidden, c.ar_hidden, c.ar_hidden, c.ar_hidden, c.ar_output};
        for (int l = 0; l < 5; ++l) {
            expect("ar_model.model." + std::to_string(2 * l) + ".weight", {dims[l + 1], dims[l]});
            expect("ar_model.model." + std::to_string(2 * l) + ".bias", {dims[l + 1]});
        }
    }
    if (c.use_spk_id) {
        expect("spk_emb_mat.weight", {c.num_spk, c.spk_emb_size});
        expect("spk_fc.weight", {c.in_channels, c.spk_emb_size});
        expect("spk_fc.bias", {c.in_channels});
    }
    if (rc != HIFICAR_OK) {
        delete h;
        return rc;
    }
    *out = h;
    return HIFICAR_OK;
}

// dst row (seq, t) = src row (seq, t / s): the nearest-upsampled copies the TRAINING forward keeps for the weight gradients (the inference
// path never materialises them).  Two tensors per launch (the raw and the ReLU'd block input); one thread = 16 bytes.
__global__ __launch_bounds__(256) static void rows_upsample2_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ da,
                                                                     float* __restrict__ db, int rows_out, int s, int c4n, long long total) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c4 = (int)(i % c4n);
        const long long row = i / c4n;
        const long long seq = row / rows_out;
        const int t = (int)(row - seq * rows_out);
        const size_t src = ((size_t)seq * (rows_out / s) + t / s) * c4n + c4;
        reinterpret_cast<f32x4*>(da)[i] = reinterpret_cast<const f32x4*>(a)[src];
        reinterpret_cast<f32x4*>(db)[i] = reinterpret_cast<const f32x4*>(b)[src];
    }
}

static int gblock_forward(hificar_handle* h, const FwdCall& k, const Ragged& rg) {
    const hificar_config& cfg = h->cfg;
    const Workspace& ws = k.ws;
    const Tape* const tp = k.tp;
    const hipStream_t stream = k.stream;
    const int B = k.B, T = k.T;
    int rc;
    const bool tapping = !h->taps.empty();
    if (tapping) {
        if ((rc = grow_tap_scratch(h, stage_elems(h, B, T))) != HIFICAR_OK) return rc;
        if (cfg.use_ar && (rc = emit_tap(h, "ar_feats", tp ? tp->xin : ws.xin, h->cin_pad, h->cf, cfg.ar_output, B, 1, 0, stream, T)) != HIFICAR_OK) return rc;
    }
    const int nb = (int)h->gb.size();
    // where GBlock i's input (raw rows, ReLU'd rows) lives at its INPUT rate: the workspace pair, or — training, scale 1 — the tape
    // slots the weight gradients read (no copy)
    auto in_raw = [&](int i) { return tp && h->gb[(size_t)i].scale == 1 ? reinterpret_cast<float*>(tp->g_xu[i]) : ws.u; };
    auto in_act = [&](int i) { return tp && h->gb[(size_t)i].scale == 1 ? tp->g_a1u[i] : ws.u_s; };
    char* const A = reinterpret_cast<char*>(ws.xt[0]);
    float* const R = ws.x[0];
    char* const Bf = reinterpret_cast<char*>(ws.xt[1]);
    {   // input conv: no activation in front of it (gblock_gen.py:128); the first GBlock consumes it raw (res1) and ReLU'd (conv1)
        const ConvLayer* lay[1] = {&h->input_conv};
        const ConvIO io[1] = {{reinterpret_cast<const char*>(tp ? tp->xin : ws.xin), nullptr, in_raw(0), in_act(0)}};
        if ((rc = launch_conv(h, lay, 1, B, T, io, 0.f, rg, stream)) != HIFICAR_OK) return rc;
        if (tapping && (rc = emit_tap(h, "input_conv", in_raw(0), stage_pad(cfg, 0), 0, cfg.channels, B, T, 0, stream)) != HIFICAR_OK) return rc;
    }
    int rows = T;
    const float* last = nullptr;
    for (int i = 0; i < nb; ++i) {
        const GBlockLayers& g = h->gb[(size_t)i];
        const int s = g.scale;
        const std::string base = "resamples." + std::to_string(i);
        const float* x_raw = in_raw(i);
        const char* x_act = in_act(i);
        int up = s;
        if (tp && s > 1) {  // training: upsampled copies for the backward pass; the convs below then read them directly
            const int c4n = g.c1a.cin_pad / 4;
            const long long total = (long long)B * rows * s * c4n;
            ProfScope prof(h, stream, "rows_upsample2_kernel", 0.0, 4.0 * B * rows * g.c1a.cin_pad * (2.0 + 2.0 * s));
            hipLaunchKernelGGL(rows_upsample2_kernel, dim3((unsigned)std::min<long long>((total + 255) / 256, 8LL * h->num_cus)), dim3(256), 0, stream, x_raw,
                               reinterpret_cast<const float*>(x_act), reinterpret_cast<float*>(tp->g_xu[i]), reinterpret_cast<float*>(tp->g_a1u[i]),
                               rows * s, s, c4n, total);
            HIP_TRY(hipGetLastError());
            x_raw = reinterpret_cast<const float*>(tp->g_xu[i]);
            x_act = tp->g_a1u[i];
            up = 1;
        }
        rows *= s;
        char* a2 = tp ? tp->g_a2[i] : A;
        char* a3 = tp ? tp->g_a3[i] : Bf;
        char* a4 = tp ? tp->g_a4[i] : A;
        {   // 1. conv1's first conv on ReLU(x) and res1's 1 x 1 conv on x: two branches over the same (upsampled) input rows
            const ConvLayer* lay[2] = {&g.c1a, &g.res};
            float* y_tap = tap_wanted(h, base + ".conv1a") ? h->tap_scratch : nullptr;
            ConvIO io[2] = {{x_act, nullptr, y_tap, a2}, {reinterpret_cast<const char*>(x_raw), nullptr, R, nullptr}};
            io[0].x_up = io[1].x_up = up;
            if ((rc = launch_conv(h, lay, 2, B, rows, io, 0.f, rg, stream)) != HIFICAR_OK) return rc;
            if (y_tap && (rc = emit_tap(h, base + ".conv1a", y_tap, g.c1a.cout_pad, 0, g.cout, B, rows, 0, stream)) != HIFICAR_OK) return rc;
            if (tapping && (rc = emit_tap(h, base + ".res1", R, g.c1a.cout_pad, 0, g.cout, B, rows, 0, stream)) != HIFICAR_OK) return rc;
        }
        {   // 2. y = conv_d3(ReLU(h1)) + r, in place over r
            const ConvLayer* lay[1] = {&g.c1b};
            const ConvIO io[1] = {{a2, R, R, a3}};
            if ((rc = launch_conv(h, lay, 1, B, rows, io, 0.f, rg, stream)) != HIFICAR_OK) return rc;
            if (tapping && (rc = emit_tap(h, base + ".mid", R, g.c1a.cout_pad, 0, g.cout, B, rows, 0, stream)) != HIFICAR_OK) return rc;
        }
        {   // 3. h3 = conv_d9(ReLU(y))
            const ConvLayer* lay[1] = {&g.c2a};
            const ConvIO io[1] = {{a3, nullptr, nullptr, a4}};
            if ((rc = launch_conv(h, lay, 1, B, rows, io, 0.f, rg, stream)) != HIFICAR_OK) return rc;
        }
        {   // 4. out = y + conv_d27(ReLU(h3)): raw + ReLU'd rows for the next GBlock, raw rows for the output conv
            const bool fin = i + 1 == nb;
            float* y = fin ? (tp ? tp->fin[0] : ws.u) : in_raw(i + 1);
            char* ys = fin ? nullptr : in_act(i + 1);
            const ConvLayer* lay[1] = {&g.c2b};
            const ConvIO io[1] = {{a4, R, y, ys}};
            if ((rc = launch_conv(h, lay, 1, B, rows, io, 0.f, rg, stream)) != HIFICAR_OK) return rc;
            if (tapping && (rc = emit_tap(h, base, y, g.c1a.cout_pad, 0, g.cout, B, rows, 0, stream)) != HIFICAR_OK) return rc;
            last = y;
        }
    }
    const float* fin[3] = {last, nullptr, nullptr};
    return launch_output_conv(h, k, rg, fin, 1, round_up(h->c_last, 32), rows);
}

// ------------------------------------------------------------------------------------------------
// backward (the generator half of articulatory/bin/train.py:241-440 for generator_type GBlockGenerator)
// ------------------------------------------------------------------------------------------------
// The adjoint of the nearest upsample + the ReLU in front of conv1, and of the un-activated res1 path:
//     dx[i, c] = [a1u[s i, c] > 0] * sum_{j < s} d1[s i + j, c]  +  sum_{j < s} d2[s i + j, c]          (fixed summation order)
// d1 = data gradient of conv1's first conv, d2 = of res1's 1 x 1 conv, both at the block's OUTPUT rate; a1u = the ReLU'd input at that rate
// (row s i of it is ReLU(x[i]), and ReLU(x) > 0 <=> x > 0).  One thread = 4 channels.
__global__ __launch_bounds__(256) static void gblock_down_kernel(const float* __restrict__ d1, const float* __restrict__ d2, const float* __restrict__ a1u,
                                                                  float* __restrict__ dx, int s, int c4n, long long total) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c4 = (int)(i % c4n);
        const long long row = i / c4n;  // (sequence, input row): output rows s * row .. s * row + s - 1 (sequences hold s times as many rows)
        const size_t o = ((size_t)row * s) * c4n + c4;
        f32x4 u = reinterpret_cast<const f32x4*>(d1)[o], v = reinterpret_cast<const f32x4*>(d2)[o];
        for (int j = 1; j < s; ++j) {
            const f32x4 p = reinterpret_cast<const f32x4*>(d1)[o + (size_t)j * c4n], q = reinterpret_cast<const f32x4*>(d2)[o + (size_t)j * c4n];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                u[e] += p[e];
                v[e] += q[e];
            }
        }
        const f32x4 m = reinterpret_cast<const f32x4*>(a1u)[o];
        f32x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = (m[e] > 0.f ? u[e] : 0.f) + v[e];
        reinterpret_cast<f32x4*>(dx)[i] = r;
    }
}

static int gblock_backward(hificar_handle* h, TrainState* ts, const Tape& tp, BwdWs& bw, DeferredReduce& pending, const float* dout, const float* out,
                           const int32_t* spk_id, int B, int T, float* grads, float* dc, float* dar, hipStream_t stream) {
    int rc;
    auto G = [&](const std::string& name) { return grads + ts->raw.offset(name); };
    Ragged rg;  // dense
    rg.frames = T;
    const int nb = (int)h->gb.size();
    int rows = T * h->hop;
    if ((rc = bwd_output_conv(h, ts, tp, bw, dout, out, B, T, rows, 1, grads, stream)) != HIFICAR_OK) return rc;  // -> bw.dm[0]
    int cur = 0;  // bw.dm[cur]: gradient of the current GBlock's output
    for (int i = nb - 1; i >= 0; --i) {
        const GBlockLayers& g = h->gb[(size_t)i];
        const ConvLayer* dg = &ts->dg_gb[(size_t)i * 5];  // data-gradient layers of c1a, c1b, res, c2a, c2b
        const int Cop = g.c1a.cout_pad, Cip = g.c1a.cin_pad, s = g.scale;
        const float* gout = bw.dm[cur];
        const float* a1u = reinterpret_cast<const float*>(tp.g_a1u[i]);
        const float* xu = reinterpret_cast<const float*>(tp.g_xu[i]);
        const float* a2 = reinterpret_cast<const float*>(tp.g_a2[i]);
        const float* a3 = reinterpret_cast<const float*>(tp.g_a3[i]);
        const float* a4 = reinterpret_cast<const float*>(tp.g_a4[i]);
        float* dh3 = bw.g1[0];
        float* dy = bw.g1[1];
        float* dh1 = bw.g1[2];
        auto wgrad = [&](const ConvLayer& L, const float* gr, const float* a, int apitch) {
            return launch_wgrad(h, L, gr, Cop, a, apitch, B, rows, G(L.name + ".weight"), bw, stream, G(L.name + ".bias"));
        };
        {   // out = y + conv_d27(a4), a4 = ReLU(h3):  dh3 = ReLU'(h3) * dgrad(dout)
            const ConvLayer* lay[1] = {&dg[4]};
            const ConvIO io[1] = {{reinterpret_cast<const char*>(gout), nullptr, dh3, nullptr, a4, 0.f}};
            if ((rc = launch_conv(h, lay, 1, B, rows, io, 0.f, rg, stream)) != HIFICAR_OK) return rc;
            if ((rc = wgrad(g.c2b, gout, a4, Cop)) != HIFICAR_OK) return rc;
        }
        {   // h3 = conv_d9(a3), a3 = ReLU(y):  dy = dout + ReLU'(y) * dgrad(dh3)
            const ConvLayer* lay[1] = {&dg[3]};
            const ConvIO io[1] = {{reinterpret_cast<const char*>(dh3), gout, dy, nullptr, a3, 0.f}};
            if ((rc = launch_conv(h, lay, 1, B, rows, io, 0.f, rg, stream)) != HIFICAR_OK) return rc;
            if ((rc = wgrad(g.c2a, dh3, a3, Cop)) != HIFICAR_OK) return rc;
        }
        {   // y = conv_d3(a2) + res1(up(x)), a2 = ReLU(h1):  dh1 = ReLU'(h1) * dgrad(dy)
            const ConvLayer* lay[1] = {&dg[1]};
            const ConvIO io[1] = {{reinterpret_cast<const char*>(dy), nullptr, dh1, nullptr, a2, 0.f}};
            if ((rc = launch_conv(h, lay, 1, B, rows, io, 0.f, rg, stream)) != HIFICAR_OK) return rc;
            if ((rc = wgrad(g.c1b, dy, a2, Cop)) != HIFICAR_OK) return rc;
            if ((rc = wgrad(g.res, dy, xu, Cip)) != HIFICAR_OK) return rc;
        }
        {   // h1 = conv(up(ReLU(x))): the two data gradients at the output rate in one launch, then the upsample's adjoint + ReLU'(x)
            if ((rc = wgrad(g.c1a, dh1, a1u, Cip)) != HIFICAR_OK) return rc;
            const ConvLayer* lay[2] = {&dg[0], &dg[2]};
            const ConvIO io[2] = {{reinterpret_cast<const char*>(dh1), nullptr, bw.dx[0], nullptr}, {reinterpret_cast<const char*>(dy), nullptr, bw.dx[1], nullptr}};
            if ((rc = launch_conv(h, lay, 2, B, rows, io, 0.f, rg, stream)) != HIFICAR_OK) return rc;
            const int rows_in = rows / s, c4n = Cip / 4;
            float* dst = i > 0 ? bw.dm[cur ^ 1] : bw.dh0;
            const long long total = (long long)B * rows_in * c4n;
            ProfScope prof(h, stream, "gblock_down_kernel", 0.0, 4.0 * B * rows_in * Cip * (3.0 * s + 1.0));
            hipLaunchKernelGGL(gblock_down_kernel, dim3((unsigned)std::min<long long>((total + 255) / 256, 8LL * h->num_cus)), dim3(256), 0, stream, bw.dx[0],
                               bw.dx[1], a1u, dst, s, c4n, total);
            HIP_TRY(hipGetLastError());
            rows = rows_in;
        }
        cur ^= 1;
        if (ts->raw.bucket_fn) {  // every gradient of GBlock i (and, for the last one, the output conv's) is enqueued: bucket done
            if ((rc = flush_reduce(h, pending, stream)) != HIFICAR_OK) return rc;
            ts->raw.bucket_fn(nb - 1 - i, stream, ts->raw.bucket_user);
        }
    }
    if ((rc = bwd_front(h, ts, tp, bw, grads, dc, dar, spk_id, nullptr, B, T, stream)) != HIFICAR_OK) return rc;
    if ((rc = flush_reduce(h, pending, stream)) != HIFICAR_OK) return rc;
    if (ts->raw.bucket_fn) ts->raw.bucket_fn(nb, stream, ts->raw.bucket_user);  // the "front" bucket
    return HIFICAR_OK;
}
