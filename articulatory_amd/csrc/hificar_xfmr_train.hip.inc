// Training of the Transformer feature model (the reference's step: articulatory/bin/train.py:241-383 through models/transformer.py:55-77 in
// train() mode): device-resident parameters, the training-mode forward with its tape, and the backward pass.
//   forward   rows -> 3 x [conv1 -> batch statistics -> normalise + ReLU -> conv2 -> batch statistics -> normalise + residual + ReLU]
//             -> w_raw_in -> elayers x [q|k|v GEMM -> attention (keeps L, dropout on P) -> w_o -> x + dropout -> LayerNorm -> linear1 (ReLU)
//             -> dropout -> linear2 -> x + dropout -> LayerNorm] -> w_out
//   backward  the same walked from the end: LayerNorm / dropout / ReLU masks elementwise, the attention's three kernels, BatchNorm's sums
//             and input gradient; every GEMM's data gradient is a conv-engine launch on its transposed pack, every weight and bias
//             gradient a launch of the weight-gradient kernels of hificar_train.hip.inc.
// Ragged batches (hificar_xfmr_forward_train_ragged): the tape keeps the frame counts and M, the number of valid frames.  Every GEMM, conv,
// data gradient and weight gradient still runs over all B T rows; what makes that right is a rule about buffers: every buffer of rows that
// such a launch reads is written by this call on every row, and on the rows of padded frames either as zeros (the outputs of the row-wise
// kernels and of the attention kernels: a k = 3 conv then sees zero padding at a sequence's own end, and a weight gradient adds 0 * finite)
// or as the finite output of a GEMM over such rows, which only a row-wise kernel or a predicate-guarded sum reads next.  DESIGN.md 3.10
// lists the buffers.  Kernels: hificar_xfmr_train_kernels.hip.h.
// Packed batches (hificar_xfmr_forward_train_packed / hificar_xfmr_backward_packed): the ragged step on Mp = sum (length + 1) rows, rounded up to
// 256, instead of B T: every sequence's frames back to back with one zero gap row behind each, so that every launch — k = 3 included — is one run
// of Mp rows; the same code path with XfmrTrainCtx::lay set.  The same buffer rule with "gap row" for "padded row".
// bf16x3 training (hificar_xfmr_set_train_precision): every forward GEMM and every data gradient — all of them XfmrTrainCtx::conv — runs the
// layer's bf16 twin (the same ConvLayer with d_w16 filled by pack16_kernel) in the engine's bf16x3 kernels, on split rows that
// xfmr_split_rows_kernel writes from the fp32 operand into one scratch buffer.  The engine is told by its precision field, set around
// the launch alone: the precision is part of the plan key, so these launches have plans of their own and every fp32 launch plans and
// runs as before.  Weight and bias gradients (XfmrTrainCtx::wgrad), the attention, the norms, the dropout and the tape are the fp32 step's.
// bf16x3w training (HIFICAR_PREC_BF16X3W): the bf16x3 step, and the weight (and bias) gradient of every layer wgrad_gemm_form selects — one tap,
// at least 128 x 128: w_raw_in, q | k | v, w_o, linear1, linear2 — in wgrad_bf16x3_kernel on rows xfmr_split_rows_t_kernel splits into two
// scratch buffers of their own (hificar_xfmr_wgrad16.hip.h); the partials and their reductions are the fp32 form's.  Every other weight
// gradient (the k = 3 convs, residual_path, w_out) is the fp32 step's.
// bf16x3wa training (HIFICAR_PREC_BF16X3WA): the bf16x3w step, and the attention's two query-tiled kernels — the forward and the backward's
// S, dPd and dQ — on bf16 MFMAs (hificar_xfmr_attn16_train.hip.h), on position tables xfmr_split_tab_kernel splits behind every parameter
// hand-over (xfmr_split_tables); the key-tiled kernels (dK, dV, the table gradient) are the fp32 step's, under a profile row of their own.
// bf16x3wac training (HIFICAR_PREC_BF16X3WAC): the bf16x3wa step, and the weight (and bias) gradient of every k = 3 conv wgrad_gemm3_form selects
// — conv_blocks.{1,2}.conv1, conv_blocks.{0,1,2}.conv2, and conv_blocks.0.conv1 where the input rows are 128 .. 1024 wide — as the one-tap GEMM
// G^T A3 in wgrad_bf16x3_kernel: A3's column k cin_pad + c of row r is row r + k - 1 of channel c within the row's own sequence
// (xfmr_split_taps_t_kernel writes it into the second of bf16x3w's two scratch buffers), the layer's one-tap twin (XfmrTrain::Bn::wg3) gives the
// launch its tiles and split count, and wreduce's gemm_cin form lays the partial out as (cout, cin, 3).
// bf16x3wack training (HIFICAR_PREC_BF16X3WACK): the bf16x3wac step, and the attention's key-tiled backward — dK, dV and the first stage of the
// table gradient — on bf16 MFMAs (hificar_xfmr_attn16_train_k.hip.h), on the banded fp32 dS / Pd xfmr_attn16_bwd_q_kernel writes: the same
// workspace and tape, profile rows xfmr_attn16_bwd_k_kernel and xfmr_demb16_partial_kernel in place of xfmr_attn_bwd_k_kernels.

struct XfmrTrainLayer {
    ConvLayer dg_qkv, dg_wo, dg_l1, dg_l2;
    int64_t off_fused = 0, off_wot = 0;  // the q | k | v weight (3 F, F) and w_o's (F, F) transpose in the master copy
};

struct XfmrTrain {
    FeatureParamTable tab;  // the master copy: the parameters, the batch norms' running statistics, the folds, the fused q | k | v and w_o^T
    float* d_wscr = nullptr;  // (3 F, F): a fused layer's weight gradient before it is unpacked
    // the batch norms in registration order: the conv in front of each, unfolded (training) and folded (eval), and where the fold lives
    struct Bn {
        std::string conv, bn;
        ConvLayer raw, dg;
        ConvLayer wg3;  // wgrad_gemm3_form(raw): the one-tap layer (cout, 3 cin_pad) whose weight gradient is raw's in bf16x3wac; else unplanned (cout 0)
        ConvLayer* folded;
        int64_t off_fw = 0, off_fb = 0;
    };
    std::vector<Bn> bns;  // sized once (launch plans are keyed by the layers' addresses)
    int bn_c1[3], bn_c2[3], bn_rp = -1;
    ConvLayer dg_win, dg_wout;
    std::vector<XfmrTrainLayer> enc;
    bool have_params = false;
    bool have16 = false;      // the bf16 fragments of every forward and data-gradient layer are allocated (the first bf16x3 training arithmetic)
    int fwd_precision = HIFICAR_PREC_F32;  // the arithmetic of the last training forward: a backward in the other one is refused
    // The packed tapes this handle filled, by address, with the frame counts their forward ran on: what lets a backward refuse, before it
    // enqueues anything, a tape of the other kind or other counts than the forward's (the tape's own header lives on the device).  A dense
    // or ragged forward into the same memory takes the entry out.
    struct PackedTape {
        int B, T;
        std::vector<int32_t> lengths;
    };
    std::map<const void*, PackedTape> packed_tapes;
};

static void xfmr_train_free(hificar_xfmr* g) {
    delete g->train;  // (device memory: the engine's allocation list)
    g->train = nullptr;
}

template <int D>
static hipError_t xfmr_train_attr() {
    static_assert(XfmrAttnLds<D>::bytes <= 160 * 1024 && XfmrEmbLds<D>::bytes <= 160 * 1024, "the attention kernels' LDS");
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&xfmr_attn_kernel<D, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)XfmrAttnLds<D>::bytes);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&xfmr_attn_bwd_q_kernel<D>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)XfmrAttnLds<D>::bytes);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&xfmr_attn_bwd_k_kernel<D>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)XfmrAttnBwdKLds<D>::bytes);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&xfmr_demb_partial_kernel<D>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)XfmrEmbLds<D>::bytes);
    if (e != hipSuccess) return e;
    if ((e = xfmr_attn16_train_attr<D>()) != hipSuccess) return e;
    return xfmr_attn16_train_k_attr<D>();
}

// the key-tiled side of the attention backward: dK, dV and the table gradient's partials, from the banded dS and Pd a query-tiled kernel wrote
template <int D>
static hipError_t xfmr_attn_bwd_k_launch(const XfmrAttnBwdParams& p, dim3 grid, float* emb_partial, int M, int chunks, hipStream_t stream) {
    hipLaunchKernelGGL((xfmr_attn_bwd_k_kernel<D>), grid, dim3(256), XfmrAttnBwdKLds<D>::bytes, stream, p);
    hipLaunchKernelGGL((xfmr_demb_partial_kernel<D>), dim3((unsigned)chunks, kXfmrHeads), dim3(256), XfmrEmbLds<D>::bytes, stream, p.qkv, p.ds, emb_partial, M,
                       p.T, p.F, p.hdr, p.lens, p.lay);
    return hipGetLastError();
}

template <int D>
static hipError_t xfmr_attn_bwd_launch(const XfmrAttnBwdParams& p, dim3 grid, float* emb_partial, int M, int chunks, hipStream_t stream) {
    hipLaunchKernelGGL((xfmr_attn_bwd_q_kernel<D>), grid, dim3(256), XfmrAttnLds<D>::bytes, stream, p);
    return xfmr_attn_bwd_k_launch<D>(p, grid, emb_partial, M, chunks, stream);
}

// what the training arithmetic switches on (kXfmrArith); x3: every bf16x3 training arithmetic has the same GEMMs and packs
static bool xfmr_train_x3(const hificar_xfmr* g) { return xfmr_arith(g->train_precision).x3; }
static bool xfmr_train_w(const hificar_xfmr* g) { return xfmr_arith(g->train_precision).w; }
static bool xfmr_train_a(const hificar_xfmr* g) { return xfmr_arith(g->train_precision).a; }
static bool xfmr_train_c(const hificar_xfmr* g) { return xfmr_arith(g->train_precision).c; }
static bool xfmr_train_k(const hificar_xfmr* g) { return xfmr_arith(g->train_precision).k; }
// three taps, one phase, at least 128 x 128, and the three taps' columns side by side fit a split buffer: the one-tap GEMM form on tap-shifted columns
static bool wgrad_gemm3_form(const ConvLayer& L) {
    return L.K == 3 && L.ntaps == 3 && L.n_phase == 1 && L.n_blocks32 >= 4 && (L.cin_pad + 31) / 32 >= 4 && 3 * L.cin_pad <= kXfmrFF;
}
static int xfmr_train_build(hificar_xfmr* g, XfmrTrain* ts);
static int xfmr_repack(hificar_xfmr* g, hipStream_t stream);
static int xfmr_split_tables(hificar_xfmr* g, hipStream_t stream);
static size_t xfmr_pack16_bytes(const ConvLayer& L);

// bf16 fragment buffers of every layer XfmrTrainCtx::conv launches (the layers' fp32 twins stay as they are), once
static int xfmr_train_alloc16(hificar_xfmr* g, XfmrTrain* ts) {
    if (ts->have16) return HIFICAR_OK;
    hificar_engine* h = &g->eng;
    std::vector<ConvLayer*> ls;
    for (auto& bn : ts->bns) {
        ls.push_back(&bn.raw);
        ls.push_back(&bn.dg);
    }
    ls.push_back(&g->w_in);
    ls.push_back(&g->w_out);
    ls.push_back(&ts->dg_win);
    ls.push_back(&ts->dg_wout);
    for (size_t l = 0; l < g->enc.size(); ++l) {
        XfmrEncLayer& L = g->enc[l];
        XfmrTrainLayer& D = ts->enc[l];
        for (ConvLayer* p : {&L.qkv, &L.wo, &L.l1, &L.l2, &D.dg_qkv, &D.dg_wo, &D.dg_l1, &D.dg_l2}) ls.push_back(p);
    }
    for (ConvLayer* L : ls) {
        if (L->d_w16) continue;
        void* p = nullptr;
        const int rc = feature_alloc(h, xfmr_pack16_bytes(*L), &p);
        if (rc != HIFICAR_OK) return rc;
        L->d_w16 = static_cast<uint16_t*>(p);
    }
    ts->have16 = true;
    return HIFICAR_OK;
}

static int xfmr_train_init(hificar_xfmr* g) {
    if (g->train) return HIFICAR_OK;
    if (!g->finalized) return fail(HIFICAR_E_STATE, "Transformer training entry points need hificar_xfmr_finalize first");
    if (g->precision != HIFICAR_PREC_F32)
        return fail(HIFICAR_E_STATE, "this Transformer handle is packed for the %s arithmetic: training and hificar_xfmr_set_parameters_device run in exact fp32 only",
                    xfmr_precision_name(g->precision));
    return feature_train_make(g, xfmr_train_build, "Transformer");
}

static int xfmr_train_build(hificar_xfmr* g, XfmrTrain* ts) {
    hificar_engine* h = &g->eng;
    const int F = g->cfg.hidden_dim, C = g->cfg.in_channels, E = g->cfg.elayers;
    const bool has_rp = g->rp.cout != 0;
    FeatureParamTable& tab = ts->tab;
    auto add = [&](const std::string& name, bool trainable) { tab.add(g->weights.expected, name, trainable); };
    // state_dict order: a module's weight and bias lie back to back (the (d gamma | d beta) pairs are reduced as one row of 2 F)
    for (int i = 0; i < 3; ++i) {
        const std::string b = "conv_blocks." + std::to_string(i) + ".";
        for (const char* m : {"conv1", "bn1", "conv2", "bn2"})
            for (const char* t : {".weight", ".bias"}) add(b + m + t, true);
        if (i == 0 && has_rp)
            for (const char* m : {"residual_path", "res_norm"})
                for (const char* t : {".weight", ".bias"}) add(b + m + t, true);
    }
    add("w_raw_in.weight", true);
    add("w_raw_in.bias", true);
    for (int l = 0; l < E; ++l) {
        const std::string b = "transformer.layers." + std::to_string(l) + ".";
        for (const char* w : {"w_q", "w_k", "w_v", "w_o"}) add(b + "self_attn." + w, true);
        add(b + "self_attn.relative_positional.embeddings", true);
        for (const char* m : {"linear1", "linear2", "norm1", "norm2"})
            for (const char* t : {".weight", ".bias"}) add(b + m + t, true);
    }
    add("w_out.weight", true);
    add("w_out.bias", true);
    tab.grad_total = tab.master_total;
    // the batch norms, in registration order
    ts->bns.resize(has_rp ? 7 : 6);
    {
        int j = 0;
        for (int i = 0; i < 3; ++i) {
            const std::string b = "conv_blocks." + std::to_string(i) + ".";
            ts->bn_c1[i] = j;
            ts->bns[(size_t)j].conv = b + "conv1";
            ts->bns[(size_t)j].bn = b + "bn1";
            ts->bns[(size_t)j++].folded = &g->c1[i];
            ts->bn_c2[i] = j;
            ts->bns[(size_t)j].conv = b + "conv2";
            ts->bns[(size_t)j].bn = b + "bn2";
            ts->bns[(size_t)j++].folded = &g->c2[i];
            if (i == 0 && has_rp) {
                ts->bn_rp = j;
                ts->bns[(size_t)j].conv = b + "residual_path";
                ts->bns[(size_t)j].bn = b + "res_norm";
                ts->bns[(size_t)j++].folded = &g->rp;
            }
        }
    }
    for (auto& bn : ts->bns) {
        add(bn.bn + ".running_mean", false);
        add(bn.bn + ".running_var", false);
    }
    for (auto& bn : ts->bns) {
        const ConvLayer& L = *bn.folded;
        bn.off_fw = tab.reserve((int64_t)L.cout * L.cin * L.K);
        bn.off_fb = tab.reserve(L.cout);
    }
    ts->enc.resize((size_t)E);
    for (auto& e : ts->enc) {
        e.off_fused = tab.reserve((int64_t)3 * F * F);
        e.off_wot = tab.reserve((int64_t)F * F);
    }
    int rc;
    void* p = nullptr;
    if ((rc = feature_alloc(h, (size_t)tab.master_total * sizeof(float), &p)) != HIFICAR_OK) return rc;
    tab.d_master = static_cast<float*>(p);
    if ((rc = feature_alloc(h, (size_t)3 * F * F * sizeof(float), &p)) != HIFICAR_OK) return rc;
    ts->d_wscr = static_cast<float*>(p);
    for (auto& bn : ts->bns) {
        const ConvLayer& L = *bn.folded;
        if ((rc = xfmr_plan(bn.raw, bn.conv + "#raw", L.cin, L.cin_pad, L.cout, L.K)) != HIFICAR_OK) return rc;
        if ((rc = feature_alloc(h, pack_w32_elems(bn.raw, bn.raw.chunk16) * sizeof(float), &p)) != HIFICAR_OK) return rc;
        bn.raw.d_w32 = static_cast<float*>(p);
        if ((rc = feature_alloc(h, (size_t)bn.raw.cout_total * sizeof(float), &p)) != HIFICAR_OK) return rc;
        bn.raw.d_bias = static_cast<float*>(p);
        if ((rc = make_dgrad_layer(h, bn.raw, bn.dg, nullptr)) != HIFICAR_OK) return rc;
        if (bn.dg.cout_pad != L.cin_pad) return fail(HIFICAR_E_INVALID, "internal: data-gradient rows of %s are %d wide, its input rows %d", bn.conv.c_str(), bn.dg.cout_pad, L.cin_pad);
        if (wgrad_gemm3_form(bn.raw)) {
            if ((rc = xfmr_plan(bn.wg3, bn.conv + "#wg3", 3 * L.cin_pad, 3 * L.cin_pad, L.cout, 1)) != HIFICAR_OK) return rc;
            if (!wgrad_gemm_form(bn.wg3) || !wgrad_gemm_wide(bn.wg3) || bn.wg3.n_blocks32 != bn.raw.n_blocks32)
                return fail(HIFICAR_E_INVALID, "internal: the one-tap twin of %s", bn.conv.c_str());
        }
    }
    (void)C;
    if ((rc = make_dgrad_layer(h, g->w_in, ts->dg_win, nullptr)) != HIFICAR_OK) return rc;
    if ((rc = make_dgrad_layer(h, g->w_out, ts->dg_wout, nullptr)) != HIFICAR_OK) return rc;
    for (int l = 0; l < E; ++l) {
        const XfmrEncLayer& L = g->enc[(size_t)l];
        XfmrTrainLayer& D = ts->enc[(size_t)l];
        if ((rc = make_dgrad_layer(h, L.qkv, D.dg_qkv, nullptr)) != HIFICAR_OK) return rc;
        if ((rc = make_dgrad_layer(h, L.wo, D.dg_wo, nullptr)) != HIFICAR_OK) return rc;
        if ((rc = make_dgrad_layer(h, L.l1, D.dg_l1, nullptr)) != HIFICAR_OK) return rc;
        if ((rc = make_dgrad_layer(h, L.l2, D.dg_l2, nullptr)) != HIFICAR_OK) return rc;
    }
    if ((rc = wgrad_setup()) != HIFICAR_OK) return rc;
    HIP_TRY(xfmr_for_every_d([](auto D) { return xfmr_train_attr<D()>(); }));
    return HIFICAR_OK;
}

extern "C" int hificar_xfmr_grad_count(hificar_xfmr* g) {
    return g && xfmr_train_init(g) == HIFICAR_OK ? (int)g->train->tab.slots.size() : -1;
}

extern "C" int hificar_xfmr_grad_info(hificar_xfmr* g, int i, char* name96, int64_t* offset, int64_t* numel) {
    if (!g || !name96 || !offset || !numel) return fail(HIFICAR_E_INVALID, "hificar_xfmr_grad_info: null argument");
    const int rc = xfmr_train_init(g);
    return rc != HIFICAR_OK ? rc : feature_grad_info(g->train->tab, i, name96, offset, numel);
}

extern "C" int64_t hificar_xfmr_grad_floats(hificar_xfmr* g) {
    return g && xfmr_train_init(g) == HIFICAR_OK ? g->train->tab.grad_total : -1;
}

static size_t xfmr_pack16_bytes(const ConvLayer& L) {
    return ((size_t)L.n_blocks32 * (L.cin_pad / L.chunk16) * L.ntaps * (L.chunk16 / 16) * 2 + 4 * (L.chunk16 / 16)) * 512 * sizeof(uint16_t);
}

// mode 0: P's own weight `w` (P.cout, P.cin, K);  mode 2: P is the data-gradient layer of the (cout, cin, K) weight `w`
static Pack16Params xfmr_pack16_params(const ConvLayer& P, const float* w, uint16_t* dst, int mode, int cin, int cout) {
    Pack16Params p;
    memset(&p, 0, sizeof(p));
    p.src = w;
    p.dst = dst;
    p.mode = mode;
    p.n_blocks32 = P.n_blocks32;
    p.nchunk = P.cin_pad / P.chunk16;
    p.ntaps = P.ntaps;
    p.nc16 = P.chunk16 / 16;
    p.chunk = P.chunk16;
    p.cin = cin;
    p.cout = cout;
    p.K = P.K;
    p.cin_pack = P.cin;
    p.cout_pack = P.cout;
    for (int t = 0; t < kPack16MaxTaps; ++t) p.tap_k[t] = t < P.ntaps ? P.tap_k[0][t] : -1;
    return p;
}

static int launch_pack16(hificar_engine* h, const Pack16Params& p, hipStream_t stream) {
    const long long n = pack16_items(p);
    ProfScope prof(h, stream, "pack16_kernel", 0.0, 4.0 * p.cin * p.cout * p.K + 2.0 * (double)pack16_frags(p) * 512);
    hipLaunchKernelGGL(pack16_kernel, dim3((unsigned)std::min<long long>((n + 255) / 256, 2048)), dim3(256), 0, stream, p);
    HIP_TRY(hipGetLastError());
    return HIFICAR_OK;
}

// forward pack (+ bias, when the layer has one) of a layer, and its data-gradient pack, from a (cout, cin, K) weight on the device.
// x3 (the bf16x3 training arithmetic): the bf16 fragments of both, and of the fp32 packs only what the eval forward reads — the forward
// pack of a layer it runs (train_only = false)
static int xfmr_pack_dev(hificar_engine* h, const ConvLayer& L, const ConvLayer* D, const float* w, const float* b, hipStream_t stream, bool x3 = false,
                         bool train_only = false) {
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
    if (!(x3 && train_only) && (rc = launch_pack(pp, stream)) != HIFICAR_OK) return rc;
    if (x3) {
        if (L.n_phase != 1 || !L.d_w16 || (D && (D->n_phase != 1 || !D->d_w16))) return fail(HIFICAR_E_INVALID, "internal: no bf16 fragments for %s", L.name.c_str());
        if ((rc = launch_pack16(h, xfmr_pack16_params(L, w, L.d_w16, 0, L.cin, L.cout), stream)) != HIFICAR_OK) return rc;
        if (D && (rc = launch_pack16(h, xfmr_pack16_params(*D, w, D->d_w16, 2, L.cin, L.cout), stream)) != HIFICAR_OK) return rc;
    }
    if (b) {
        PackParams pb = simple_pack(6, b, L.d_bias, (long long)L.n_phase * L.cout);
        pb.cout = L.cout;
        pb.cout_pad = L.cout_pad;
        if ((rc = launch_pack(pb, stream)) != HIFICAR_OK) return rc;
    }
    if (D && !x3) {
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

extern "C" int hificar_xfmr_set_parameters_device(hificar_xfmr* g, const char* const* names, const float* const* data, int n, void* stream_) {
    if (!g || !names || !data) return fail(HIFICAR_E_INVALID, "hificar_xfmr_set_parameters_device: null argument");
    int rc = xfmr_train_init(g);
    if (rc != HIFICAR_OK) return rc;
    XfmrTrain* ts = g->train;
    hificar_engine* h = &g->eng;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if ((rc = enter_stream(h, stream)) != HIFICAR_OK) return rc;
    if ((rc = feature_upload(g->weights.expected, ts->tab, names, data, n, "hificar_xfmr_set_parameters_device", stream)) != HIFICAR_OK) return rc;
    if ((rc = xfmr_repack(g, stream)) != HIFICAR_OK) return rc;
    ts->have_params = true;
    return HIFICAR_OK;
}

// every pack the handle's arithmetics read, from the master copy, on `stream`
static int xfmr_repack(hificar_xfmr* g, hipStream_t stream) {
    XfmrTrain* ts = g->train;
    hificar_engine* h = &g->eng;
    int rc;
    const bool x3 = xfmr_train_x3(g);
    if (x3 && (rc = xfmr_train_alloc16(g, ts)) != HIFICAR_OK) return rc;
    const int F = g->cfg.hidden_dim, d = F / kXfmrHeads;
    float* const m = ts->tab.d_master;
    auto at = [&](const std::string& name) { return ts->tab.at(name); };
    for (auto& bn : ts->bns) {
        const ConvLayer& L = *bn.folded;
        if ((rc = xfmr_pack_dev(h, bn.raw, &bn.dg, at(bn.conv + ".weight"), at(bn.conv + ".bias"), stream, x3, true)) != HIFICAR_OK) return rc;
        hipLaunchKernelGGL(xfmr_fold_kernel, dim3((unsigned)L.cout), dim3(256), 0, stream, at(bn.conv + ".weight"), at(bn.conv + ".bias"), at(bn.bn + ".weight"),
                           at(bn.bn + ".bias"), at(bn.bn + ".running_mean"), at(bn.bn + ".running_var"), m + bn.off_fw, m + bn.off_fb, L.cin * L.K);
        HIP_TRY(hipGetLastError());
        if ((rc = xfmr_pack_dev(h, L, nullptr, m + bn.off_fw, m + bn.off_fb, stream)) != HIFICAR_OK) return rc;
    }
    if ((rc = xfmr_pack_dev(h, g->w_in, &ts->dg_win, at("w_raw_in.weight"), at("w_raw_in.bias"), stream, x3)) != HIFICAR_OK) return rc;
    if ((rc = xfmr_pack_dev(h, g->w_out, &ts->dg_wout, at("w_out.weight"), at("w_out.bias"), stream, x3)) != HIFICAR_OK) return rc;
    for (int l = 0; l < g->cfg.elayers; ++l) {
        const std::string b = "transformer.layers." + std::to_string(l) + ".";
        XfmrEncLayer& L = g->enc[(size_t)l];
        XfmrTrainLayer& D = ts->enc[(size_t)l];
        hipLaunchKernelGGL(xfmr_qkv_weight_kernel, dim3(1024), dim3(256), 0, stream, at(b + "self_attn.w_q"), at(b + "self_attn.w_k"), at(b + "self_attn.w_v"),
                           m + D.off_fused, F, d, 0);
        hipLaunchKernelGGL(transpose_kernel, dim3(1024), dim3(256), 0, stream, at(b + "self_attn.w_o"), m + D.off_wot, F, F);
        HIP_TRY(hipGetLastError());
        if ((rc = xfmr_pack_dev(h, L.qkv, &D.dg_qkv, m + D.off_fused, nullptr, stream, x3)) != HIFICAR_OK) return rc;
        if ((rc = xfmr_pack_dev(h, L.wo, &D.dg_wo, m + D.off_wot, nullptr, stream, x3)) != HIFICAR_OK) return rc;
        if ((rc = xfmr_pack_dev(h, L.l1, &D.dg_l1, at(b + "linear1.weight"), at(b + "linear1.bias"), stream, x3)) != HIFICAR_OK) return rc;
        if ((rc = xfmr_pack_dev(h, L.l2, &D.dg_l2, at(b + "linear2.weight"), at(b + "linear2.bias"), stream, x3)) != HIFICAR_OK) return rc;
        HIP_TRY(hipMemcpyAsync(L.d_emb, at(b + "self_attn.relative_positional.embeddings"), (size_t)kXfmrHeads * kXfmrTab * d * sizeof(float),
                               hipMemcpyDeviceToDevice, stream));
        int i = 0;
        for (const char* nm : {"norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias"})
            HIP_TRY(hipMemcpyAsync(L.d_ln[i++], at(b + nm), (size_t)F * sizeof(float), hipMemcpyDeviceToDevice, stream));
    }
    if (xfmr_train_a(g)) return xfmr_split_tables(g, stream);
    return HIFICAR_OK;
}

// bf16x3wa: every layer's position table as the attention's MFMA operand ([hi, lo][8][208][d] bf16, rows 199 .. 207 zeros), from the
// handle's fp32 copy, on `stream` — behind every parameter hand-over (xfmr_repack) and behind a switch to this arithmetic
static int xfmr_split_tables(hificar_xfmr* g, hipStream_t stream) {
    hificar_engine* h = &g->eng;
    const int d = g->cfg.hidden_dim / kXfmrHeads;
    const size_t n = (size_t)kXfmrHeads * kXfmrTabPad * d;
    for (XfmrEncLayer& L : g->enc) {
        if (!L.d_emb16) {
            void* p = nullptr;
            const int rc = feature_alloc(h, 2 * n * sizeof(uint16_t), &p);
            if (rc != HIFICAR_OK) return rc;
            L.d_emb16 = static_cast<uint16_t*>(p);
        }
        ProfScope prof(h, stream, "xfmr_split_tab_kernel", 0.0, 8.0 * n);
        hipLaunchKernelGGL(xfmr_split_tab_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, L.d_emb, L.d_emb16, L.d_emb16 + n, d);
        HIP_TRY(hipGetLastError());
    }
    return HIFICAR_OK;
}

// The arithmetic of the training step's forward and data-gradient GEMMs; see include/hificar.h.  Before the training state exists it only
// records the choice.  Afterwards the packs of the new arithmetic are rebuilt from the master copy, behind the handle's last call.
extern "C" int hificar_xfmr_set_train_precision(hificar_xfmr* g, int precision) {
    if (!g) return fail(HIFICAR_E_INVALID, "hificar_xfmr_set_train_precision: null handle");
    const XfmrArith* to = xfmr_arith_find(precision);
    if (!to || !to->train) return fail(HIFICAR_E_INVALID, "unknown training precision %d", precision);
    if (g->precision != HIFICAR_PREC_F32)
        return fail(HIFICAR_E_STATE, "this Transformer handle is packed for the %s inference arithmetic: it has no training step, in either arithmetic",
                    xfmr_precision_name(g->precision));
    if (precision == g->train_precision) return HIFICAR_OK;
    // (among bf16x3, bf16x3w, bf16x3wa, bf16x3wac and bf16x3wack: the same packs, other weight-gradient or attention kernels; towards one of the
    // last three from one of the first two the tables are split)
    const bool same_packs = to->x3 && xfmr_train_x3(g);
    if (!g->train || !g->train->have_params || (same_packs && (!to->a || xfmr_train_a(g)))) {
        g->train_precision = precision;
        return HIFICAR_OK;
    }
    hificar_engine* h = &g->eng;
    hipStream_t stream = h->have_last_stream ? h->last_stream : nullptr;
    int rc = enter_stream(h, stream);
    if (rc != HIFICAR_OK) return rc;
    const int before = g->train_precision;
    g->train_precision = precision;
    if ((rc = same_packs ? xfmr_split_tables(g, stream) : xfmr_repack(g, stream)) != HIFICAR_OK) g->train_precision = before;
    return rc;
}

// ------------------------------------------------------------------------------------------------
// tape and workspace
// ------------------------------------------------------------------------------------------------
// Mp of a packed batch: every sequence's frames and one gap row behind each, rounded up to kXfmrPackGranule rows (the tail: gap rows).
// 256 = kXfmrColRows = kXfmrEmbRows: whole chunks for the column sums and the table gradient, and few distinct row counts per length
// bucket for the conv engine's plan cache, which is keyed by the row count.  0: a length outside 0 .. T, or fewer than two frames.
constexpr int kXfmrPackGranule = 256;
static long long xfmr_packed_rows(int B, int T, const int32_t* lengths_host, long long* valid = nullptr) {
    if (B < 1 || T < 1 || !lengths_host) return 0;
    long long m = 0;
    for (int b = 0; b < B; ++b) {
        if (lengths_host[b] < 0 || lengths_host[b] > T) return 0;
        m += lengths_host[b];
    }
    if (valid) *valid = m;
    if (m < 2) return 0;
    return (m + B + kXfmrPackGranule - 1) / kXfmrPackGranule * kXfmrPackGranule;
}

struct XfmrTapeLayer {
    float *qkv, *o, *lse, *p1, *n1, *hid, *p2;
};

struct XfmrTape {
    BigruTapeHeader* hdr;
    float* xin;       // [rows][cin_pad]
    float* y[7];      // per batch norm: its conv's raw output rows [rows][F]
    float* stats[7];  // ... and mean | biased variance | rstd, [3][F]
    float* a1[3];     // per ResBlock: relu(bn1(conv1))
    float* bo[3];     // ... and its output
    std::vector<float*> X;  // [elayers + 1]: the encoder layers' inputs, and the last one's output
    std::vector<XfmrTapeLayer> L;
    int* lens;  // [B] frame counts of a ragged forward (the header says whether they hold)
    int *row0, *pad_row;  // a packed forward's tables, [B + 1] and [Mp] (XfmrLayout); null otherwise
    size_t bytes;
};

// Mp = 0: the rows of the padded batch (dense, ragged); Mp > 0: a packed batch of Mp rows (T plays no part)
static XfmrTape xfmr_plan_tape(const hificar_xfmr* g, int B, int T, void* base, int Mp = 0) {
    const size_t rows = Mp ? (size_t)Mp : feature_train_rows(B, T), F = (size_t)g->cfg.hidden_dim;  // (Mp: a multiple of 256 already, as the eval path's rows)
    const int nbn = g->rp.cout ? 7 : 6;
    Carver cv(base, 256);
    XfmrTape t;
    t.hdr = cv.take<BigruTapeHeader>(256);
    t.xin = cv.floats(rows * g->cin_pad);
    for (int j = 0; j < 7; ++j) {
        t.y[j] = j < nbn ? cv.floats(rows * F) : nullptr;
        t.stats[j] = j < nbn ? cv.floats(3 * F) : nullptr;
    }
    for (int i = 0; i < 3; ++i) {
        t.a1[i] = cv.floats(rows * F);
        t.bo[i] = cv.floats(rows * F);
    }
    const int E = g->cfg.elayers;
    t.X.resize((size_t)E + 1);
    t.L.resize((size_t)E);
    for (int l = 0; l <= E; ++l) t.X[(size_t)l] = cv.floats(rows * F);
    for (int l = 0; l < E; ++l) {
        XfmrTapeLayer& L = t.L[(size_t)l];
        L.qkv = cv.floats(rows * 3 * F);
        L.o = cv.floats(rows * F);
        L.lse = cv.floats(rows * kXfmrHeads);
        L.p1 = cv.floats(rows * F);
        L.n1 = cv.floats(rows * F);
        L.hid = cv.floats(rows * kXfmrFF);
        L.p2 = cv.floats(rows * F);
    }
    t.lens = cv.take<int>((size_t)B * sizeof(int));
    t.row0 = Mp ? cv.take<int>(((size_t)B + 1) * sizeof(int)) : nullptr;
    t.pad_row = Mp ? cv.take<int>((size_t)Mp * sizeof(int)) : nullptr;
    t.bytes = cv.bytes();
    return t;
}

struct XfmrTrainWs {
    float* t1;       // [rows][F]: a sub-block's output before its dropout
    float* res;      // [rows][F]: res_norm's rows
    float* d[3];     // [rows][F]: gradient rows
    float* wide;     // [rows][3072]: dropout(hidden rows); w_out's rows; dout as rows
    float* gw;       // [rows][3072]: gradient of the hidden rows; dq | dk | dv
    float* dxr[2];   // [rows][cin_pad]
    float* ds;       // [B][8][T][200] banded dS (packed: [Mp][8][200])
    float* pd;       // ... and the dropped probabilities
    float* rowstats; // [rows][2]
    float* colpart;  // [chunks][2][F]
    float* embpart;  // [chunks][8][199][d]
    float* partial;  // weight-gradient partials
    float* colsum;   // bias-gradient partials
    char* light;     // a forward without a tape keeps its rows here
    char* split;     // [rows][3072] split rows (4 bytes per channel): the operand of the next bf16x3 GEMM; null in the fp32 arithmetic
    char* split_t[2];  // [rows / 8][3072][32 bytes]: G and A of the next bf16x3w weight gradient (xfmr_split_rows_t_kernel), or G and the
                       // tap-shifted A3 of a k = 3 conv's in bf16x3wac (xfmr_split_taps_t_kernel: 3 cin_pad <= 3072 columns); null otherwise
    size_t partial_elems, colsum_elems;
    size_t bytes;
};

static XfmrTrainWs xfmr_plan_train_ws(const hificar_xfmr* g, int B, int T, void* base, int Mp = 0) {
    const int M = Mp ? Mp : B * T;
    const size_t rows = Mp ? (size_t)Mp : feature_train_rows(B, T), F = (size_t)g->cfg.hidden_dim;
    Carver cv(base, 256);
    XfmrTrainWs w;
    w.t1 = cv.floats(rows * F);
    w.res = cv.floats(rows * F);
    for (int i = 0; i < 3; ++i) w.d[i] = cv.floats(rows * F);
    w.wide = cv.floats(rows * kXfmrFF);
    w.gw = cv.floats(rows * kXfmrFF);
    for (int i = 0; i < 2; ++i) w.dxr[i] = cv.floats(rows * g->cin_pad);
    w.ds = cv.floats(rows * kXfmrHeads * kXfmrBand);
    w.pd = cv.floats(rows * kXfmrHeads * kXfmrBand);
    w.rowstats = cv.floats(rows * 2);
    w.colpart = cv.floats((size_t)((M + kXfmrColRows - 1) / kXfmrColRows) * 2 * F);
    w.embpart = cv.floats((size_t)((M + kXfmrEmbRows - 1) / kXfmrEmbRows) * kXfmrTab * F);
    w.partial_elems = w.colsum_elems = 0;
    if (g->train) {
        const hificar_engine* h = &g->eng;
        auto one = [&](const ConvLayer& L, int nseq, int r) {
            w.partial_elems = std::max(w.partial_elems, wgrad_partial_elems(h, L, nseq, r));
            w.colsum_elems = std::max(w.colsum_elems, wgrad_colsum_elems(h, L, nseq, r));
        };
        for (const auto& bn : g->train->bns) {
            one(bn.raw, bn.raw.K > 1 && !Mp ? B : 1, bn.raw.K > 1 && !Mp ? T : M);
            if (xfmr_train_c(g) && bn.wg3.cout) one(bn.wg3, 1, M);  // (the GEMM form's split count, not the taps form's)
        }
        one(g->w_in, 1, M);
        one(g->w_out, 1, M);
        for (const auto& L : g->enc) {
            one(L.qkv, 1, M);
            one(L.wo, 1, M);
            one(L.l1, 1, M);
            one(L.l2, 1, M);
        }
    }
    w.partial = cv.floats(w.partial_elems);
    w.colsum = cv.floats(w.colsum_elems);
    w.light = cv.take<char>(xfmr_plan_tape(g, B, T, nullptr, Mp).bytes);
    // (last: everything in front of it lies where the fp32 arithmetic has it)
    w.split = xfmr_train_x3(g) ? cv.floats<char>(rows * kXfmrFF) : nullptr;
    for (char*& s : w.split_t)  // (behind it: a bf16x3 workspace is a prefix of the bf16x3w one; bf16x3wa's and bf16x3wac's are bf16x3w's)
        s = xfmr_train_w(g) ? cv.take<char>((size_t)split_t_bytes((long long)rows, kXfmrFF)) : nullptr;
    w.bytes = cv.bytes();
    return w;
}

extern "C" size_t hificar_xfmr_tape_bytes(const hificar_xfmr* g, int B, int T) {
    if (!g || !g->finalized || B < 1 || T < 1) return 0;
    return xfmr_plan_tape(g, B, T, nullptr).bytes;
}

extern "C" size_t hificar_xfmr_train_workspace_bytes(hificar_xfmr* g, int B, int T) {
    if (!g || B < 1 || T < 1 || xfmr_train_init(g) != HIFICAR_OK) return 0;
    return xfmr_plan_train_ws(g, B, T, nullptr).bytes;
}

static bool xfmr_packed_size_ok(int B, int Mp) {
    return B >= 1 && B <= 65535 && Mp >= kXfmrPackGranule && Mp % kXfmrPackGranule == 0 && (long long)Mp * kXfmrFF < (1LL << 31);
}

extern "C" int hificar_xfmr_packed_rows(int B, int T, const int32_t* lengths_host) {
    const long long mp = xfmr_packed_rows(B, T, lengths_host);
    return mp * kXfmrFF < (1LL << 31) ? (int)mp : 0;
}

extern "C" size_t hificar_xfmr_tape_bytes_packed(const hificar_xfmr* g, int B, int Mp) {
    if (!g || !g->finalized || !xfmr_packed_size_ok(B, Mp)) return 0;
    return xfmr_plan_tape(g, B, 0, nullptr, Mp).bytes;
}

extern "C" size_t hificar_xfmr_train_workspace_bytes_packed(hificar_xfmr* g, int B, int Mp) {
    if (!g || !xfmr_packed_size_ok(B, Mp) || xfmr_train_init(g) != HIFICAR_OK) return 0;
    return xfmr_plan_train_ws(g, B, 0, nullptr, Mp).bytes;
}

static int xfmr_train_check(hificar_xfmr* g, const char* what, int B, int T, void* tape, size_t tape_bytes, void* workspace, size_t workspace_bytes,
                            bool tape_optional = false, int Mp = 0) {
    if (!g) return fail(HIFICAR_E_INVALID, "%s: null handle", what);
    int rc = xfmr_train_init(g);
    if (rc != HIFICAR_OK) return rc;
    if (!g->train->have_params) return fail(HIFICAR_E_STATE, "%s before hificar_xfmr_set_parameters_device", what);
    if (Mp) {  // packed: the row-major indices are those of Mp rows; the padded index b T + t only has to fit an int
        if (B < 1 || T < 1 || (long long)B * T > (1LL << 30) / 8 || !xfmr_packed_size_ok(B, Mp))
            return fail(HIFICAR_E_INVALID, "%s: B=%d, T=%d, %d packed rows out of range (packed rows * 3072 < 2^31)", what, B, T, Mp);
    } else if (B < 1 || T < 1 || B > 65535 || (long long)B * T > (1LL << 30) / 8 || (long long)B * T * kXfmrFF >= (1LL << 31))
        return fail(HIFICAR_E_INVALID, "%s: B=%d, T=%d out of range (B T 3072 < 2^31)", what, B, T);
    if ((long long)B * T < 2) return fail(HIFICAR_E_INVALID, "%s: batch statistics need more than one frame (B * T = 1)", what);
    if ((!tape && !tape_optional) || reinterpret_cast<uintptr_t>(tape) % 256 || !workspace || reinterpret_cast<uintptr_t>(workspace) % 256)
        return fail(HIFICAR_E_INVALID, "%s: tape and workspace must be 256-byte aligned device pointers", what);
    const size_t tb = xfmr_plan_tape(g, B, T, nullptr, Mp).bytes, wb = xfmr_plan_train_ws(g, B, T, nullptr, Mp).bytes;
    if (tape && tape_bytes < tb) return fail(HIFICAR_E_WORKSPACE, "%s: tape too small: %zu < %zu", what, tape_bytes, tb);
    return check_workspace_size(what, workspace_bytes, wb);
}

// The launches both passes are made of
struct XfmrTrainCtx {
    hificar_xfmr* g;
    hificar_engine* h;
    hipStream_t stream;
    int B, T, M, F;  // M = B T: the rows of the padded batch (the valid ones are counted by the tape's header); packed: Mp
    const BigruTapeHeader* hdr;
    const int* lens;      // the tape's frame counts (the kernels honour them when the header says ragged)
    const int* fwd_lens;  // the same for the kernels the eval path shares, which take no header: null in a dense forward
    const XfmrTrainWs* ws;
    BwdWs bw;
    XfmrLayout lay;  // the packed form's tables: every GEMM is then one run of M rows, K = 3 included (the gap rows are the sequences' ends)
    bool packed() const { return lay.pad_row != nullptr; }

    unsigned ew_grid(long long n) const { return (unsigned)std::min<long long>((n / 4 + 255) / 256, 4096); }
    // one launch of one layer over B sequences of T rows (K = 3: the sequences' own ends) or, seq = false, over the B T rows as one
    int conv(const ConvLayer& L, const float* xs, const float* res, float* y, float* ys, bool seq = true) const {
        ConvIO io{};
        io.xs = reinterpret_cast<const char*>(xs);
        io.res = res;
        io.y = y;
        io.ys = reinterpret_cast<char*>(ys);
        const Ragged rg;
        if (!x3()) return seq && !packed() ? launch_conv1(h, L, B, T, io, 0.f, rg, stream) : launch_conv1(h, L, 1, M, io, 0.f, rg, stream);
        // bf16x3: the operand as split rows, the layer's bf16 twin in the engine's bf16x3 kernels.  Their activated copy is split rows, so a
        // ReLU'd fp32 copy (linear1's hidden rows) is the fp32 output ReLU'd in place.
        if (!L.d_w16 || !ws->split || (y && ys)) return fail(HIFICAR_E_INVALID, "internal: bf16x3 training launch of %s", L.name.c_str());
        int rc;
        if ((rc = split_rows(xs, L.cin_pad)) != HIFICAR_OK) return rc;
        io.xs = ws->split;
        io.ys = nullptr;
        if (ys) io.y = ys;
        h->precision = HIFICAR_PREC_BF16X3;  // (part of the plan key: these launches' plans are their own)
        rc = seq && !packed() ? launch_conv1(h, L, B, T, io, 0.f, rg, stream) : launch_conv1(h, L, 1, M, io, 0.f, rg, stream);
        h->precision = HIFICAR_PREC_F32;
        if (rc != HIFICAR_OK || !ys) return rc;
        return gate(ys, ys, ys, (long long)M * L.cout_pad, -1);
    }
    bool x3() const { return xfmr_train_x3(g); }
    // one profile row of attention launches at head size d: launch(std::integral_constant<int, D>) enqueues them
    template <class Launch>
    int attn(const char* row, double flops, double bytes, const char* what, int d, Launch&& launch) const {
        ProfScope prof(h, stream, row, flops, bytes);
        const hipError_t e = xfmr_by_d(d, launch);
        if (e != hipSuccess) return fail(HIFICAR_E_HIP, "%s launch failed: %s", what, hipGetErrorString(e));
        return HIFICAR_OK;
    }
    // fp32 rows [M][C] -> the split scratch (rows of padded frames and gap rows: zero bits, not read)
    int split_rows(const float* x, int C) const {
        const long long n8 = (long long)M * C / 8;
        ProfScope prof(h, stream, "xfmr_split_rows_kernel", 0.0, 8.0 * M * C);
        hipLaunchKernelGGL(xfmr_split_rows_kernel, dim3((unsigned)std::min<long long>((n8 + 255) / 256, 8192)), dim3(256), 0, stream, x, ws->split, n8, C, hdr, lens,
                           T, lay);
        HIP_TRY(hipGetLastError());
        return HIFICAR_OK;
    }
    // fp32 rows [M][C] -> 8-row groups of split columns (rows of padded frames and gap rows: zero bits, not read)
    int split_rows_t(const float* x, int C, char* dst) const {
        const long long n = split_t_items(M, C);
        ProfScope prof(h, stream, "xfmr_split_rows_t_kernel", 0.0, 8.0 * M * C);
        hipLaunchKernelGGL(xfmr_split_rows_t_kernel, dim3((unsigned)std::min<long long>((n + 255) / 256, 8192)), dim3(256), 0, stream, x, dst, (long long)M, C, hdr,
                           lens, T, lay);
        HIP_TRY(hipGetLastError());
        return HIFICAR_OK;
    }
    // fp32 rows [M][C] -> 8-row groups of 3 C split columns, tap k's at k C: row r + k - 1 of the row's own sequence, zero bits outside it
    int split_taps_t(const float* x, int C, char* dst) const {
        const long long n = split_t3_items(M, C);
        ProfScope prof(h, stream, "xfmr_split_taps_t_kernel", 0.0, 16.0 * M * C);
        hipLaunchKernelGGL(xfmr_split_taps_t_kernel, dim3((unsigned)std::min<long long>((n + 255) / 256, 8192)), dim3(256), 0, stream, x, dst, (long long)M, C, hdr,
                           lens, T, lay);
        HIP_TRY(hipGetLastError());
        return HIFICAR_OK;
    }
    // g3: the layer's one-tap twin (XfmrTrain::Bn::wg3), where it has one
    int wgrad(const ConvLayer& L, const float* gr, int gpitch, const float* a, int apitch, float* dW, float* db, const ConvLayer* g3 = nullptr) const {
        if (xfmr_train_c(g) && g3 && g3->cout) {  // bf16x3wac: a wide k = 3 conv as the one-tap GEMM G^T A3 on bf16 MFMAs
            if (!ws->split_t[0] || !ws->split_t[1] || gpitch > kXfmrFF || apitch != L.cin_pad || g3->cin_pad != 3 * apitch || 3 * apitch > kXfmrFF)
                return fail(HIFICAR_E_INVALID, "internal: bf16x3wac weight gradient of %s", L.name.c_str());
            int rc;
            if ((rc = split_rows_t(gr, gpitch, ws->split_t[0])) != HIFICAR_OK || (rc = split_taps_t(a, apitch, ws->split_t[1])) != HIFICAR_OK) return rc;
            WgradJob job = {g3, gr, gpitch, a, 3 * apitch, dW, db};
            job.gemm_cin = L.cin;
            job.gemm_kt = 3;
            job.gemm_pitch = L.cin_pad != L.cin ? L.cin_pad : 0;
            job.shape = &L;
            job.g16 = ws->split_t[0];
            job.a16 = ws->split_t[1];
            return launch_wgrad_n(h, &job, 1, 1, M, bw, stream);
        }
        if (xfmr_train_w(g) && wgrad_gemm_form(L)) {  // bf16x3w, bf16x3wa: the one-tap GEMM form on bf16 MFMAs
            if (!ws->split_t[0] || !ws->split_t[1] || gpitch > kXfmrFF || apitch > kXfmrFF) return fail(HIFICAR_E_INVALID, "internal: bf16x3w weight gradient of %s", L.name.c_str());
            int rc;
            if ((rc = split_rows_t(gr, gpitch, ws->split_t[0])) != HIFICAR_OK || (rc = split_rows_t(a, apitch, ws->split_t[1])) != HIFICAR_OK) return rc;
            WgradJob job = {&L, gr, gpitch, a, apitch, dW, db};
            job.g16 = ws->split_t[0];
            job.a16 = ws->split_t[1];
            return launch_wgrad_n(h, &job, 1, 1, M, bw, stream);
        }
        return L.K > 1 && !packed() ? launch_wgrad(h, L, gr, gpitch, a, apitch, B, T, dW, bw, stream, db)
                                    : launch_wgrad(h, L, gr, gpitch, a, apitch, 1, M, dW, bw, stream, db);
    }
    int colsum(int mode, const float* x, const float* dy, const float* stats) const {
        XfmrColParams p;
        p.x = x;
        p.dy = dy;
        p.stats = stats;
        p.rowstats = ws->rowstats;
        p.partial = ws->colpart;
        p.hdr = hdr;
        p.lens = lens;
        p.M = M;
        p.T = T;
        p.F = F;
        p.mode = mode;
        p.lay = lay;
        hipLaunchKernelGGL(xfmr_colsum_kernel, dim3((unsigned)(F / 64), (unsigned)chunks()), dim3(256), 0, stream, p);
        HIP_TRY(hipGetLastError());
        return HIFICAR_OK;
    }
    int chunks() const { return (M + kXfmrColRows - 1) / kXfmrColRows; }
    // partial (d gamma | d beta) -> the gradient buffer (the two tensors lie back to back)
    int pair_reduce(float* dgamma) const {
        hipLaunchKernelGGL(bigru_colreduce_kernel, dim3((unsigned)((2 * F + 255) / 256)), dim3(256), 0, stream, ws->colpart, chunks(), 2 * F, dgamma);
        HIP_TRY(hipGetLastError());
        return HIFICAR_OK;
    }
    int bn_stats(const float* y, float* stats, float* batch_stats) const {
        ProfScope prof(h, stream, "xfmr_bn_stats_kernels", 0.0, 8.0 * M * F);
        int rc;
        if ((rc = colsum(0, y, nullptr, nullptr)) != HIFICAR_OK) return rc;
        hipLaunchKernelGGL(xfmr_bn_mean_kernel, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, stream, ws->colpart, chunks(), F, hdr, stats);
        if ((rc = colsum(1, y, nullptr, stats)) != HIFICAR_OK) return rc;
        hipLaunchKernelGGL(xfmr_bn_var_kernel, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, stream, ws->colpart, chunks(), F, hdr, stats, batch_stats);
        HIP_TRY(hipGetLastError());
        return HIFICAR_OK;
    }
    int bn_apply(const float* y, const float* stats, const float* gamma, const float* res, float* out, bool relu) const {
        const long long n4 = (long long)M * F / 4;
        ProfScope prof(h, stream, "xfmr_bn_apply_kernel", 0.0, 4.0 * M * F * (res ? 3 : 2));
        hipLaunchKernelGGL(xfmr_bn_apply_kernel, dim3(ew_grid(4 * n4)), dim3(256), 0, stream, y, stats, gamma, gamma + F, res, out, n4, F, relu ? 1 : 0,
                           fwd_lens, T, lay);
        HIP_TRY(hipGetLastError());
        return HIFICAR_OK;
    }
    // dy -> dx (may be the same rows), d gamma | d beta into the gradient buffer at dgamma
    int bn_bwd(const float* y, const float* dy, const float* stats, const float* gamma, float* dgamma, float* dx) const {
        ProfScope prof(h, stream, "xfmr_bn_bwd_kernels", 0.0, 20.0 * M * F);
        int rc;
        if ((rc = colsum(2, y, dy, stats)) != HIFICAR_OK) return rc;
        if ((rc = pair_reduce(dgamma)) != HIFICAR_OK) return rc;
        const long long n = (long long)M * F;
        hipLaunchKernelGGL(xfmr_bn_bwd_dx_kernel, dim3(ew_grid(n)), dim3(256), 0, stream, y, dy, stats, gamma, dgamma, dgamma + F, dx, n, F, hdr, lens, T, lay);
        HIP_TRY(hipGetLastError());
        return HIFICAR_OK;
    }
    int layer_norm(const float* src, const float* gamma, const float* beta, float* dst) const {
        XfmrLnParams p;
        p.x = src;
        p.gamma = gamma;
        p.beta = beta;
        p.lengths = fwd_lens;
        p.zero_pad = 1;  // the next GEMM and its weight gradient read every row
        p.y = dst;
        p.B = packed() ? 1 : B;
        p.T = packed() ? M : T;
        p.F = F;
        p.pad_row = lay.pad_row;
        ProfScope prof(h, stream, "xfmr_ln_kernel", 8.0 * M * F, 8.0 * M * F);
        hipLaunchKernelGGL(xfmr_ln_kernel<false>, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, stream, p);
        HIP_TRY(hipGetLastError());
        return HIFICAR_OK;
    }
    int ln_bwd(const float* x, const float* dy, const float* gamma, float* dgamma, float* dx) const {
        ProfScope prof(h, stream, "xfmr_ln_bwd_kernels", 16.0 * M * F, 20.0 * M * F);
        int rc;
        // (dx is never dy here: the column sums below still read dy; the first pass leaves the row statistics for them)
        hipLaunchKernelGGL(xfmr_ln_bwd_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, stream, x, dy, gamma, dx, ws->rowstats, (long long)M, F, hdr,
                           lens, T, lay);
        HIP_TRY(hipGetLastError());
        if ((rc = colsum(3, x, dy, nullptr)) != HIFICAR_OK) return rc;
        return pair_reduce(dgamma);
    }
    int add_drop(const float* x, const float* t, float* out, int site) const {
        const long long n = (long long)M * F;
        ProfScope prof(h, stream, "xfmr_add_drop_kernel", 0.0, 12.0 * n);
        hipLaunchKernelGGL(xfmr_add_drop_kernel, dim3(ew_grid(n)), dim3(256), 0, stream, x, t, out, n, hdr, site, lens, F, T, lay);
        HIP_TRY(hipGetLastError());
        return HIFICAR_OK;
    }
    // out = (a > 0 ? d : 0) * dropout factor of `site` (a = null: no ReLU mask; site < 0: no dropout)
    int gate(const float* a, const float* dsrc, float* out, long long n, int site) const {
        ProfScope prof(h, stream, "xfmr_gate_kernel", 0.0, 4.0 * n * (a ? 3 : 2));
        hipLaunchKernelGGL(xfmr_gate_kernel, dim3(ew_grid(n)), dim3(256), 0, stream, a, dsrc, out, n, hdr, site, lens, (int)(n / M), T, lay);
        HIP_TRY(hipGetLastError());
        return HIFICAR_OK;
    }
    // packed: zeros in the gap rows of rows written by a kernel that writes a sequence's own rows only
    int zero_gaps(float* rows, int width) const {
        if (!packed()) return HIFICAR_OK;
        hipLaunchKernelGGL(xfmr_zero_gaps_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, stream, rows, width, lay.pad_row, M);
        HIP_TRY(hipGetLastError());
        return HIFICAR_OK;
    }
};

#define XT(call)                                  \
    do {                                          \
        if ((rc = (call)) != HIFICAR_OK) return rc; \
    } while (0)

// Transformer.forward in train() mode; see include/hificar.h.  tape = NULL: the rows a tape would keep live in the workspace.
// Test aid (hificar_xfmr_debug_tap): the ReLU outputs, as rows — "conv_blocks.<n>.relu1", "conv_blocks.<n>.relu2" (B, T, hidden_dim) and
// "layers.<n>.hidden" (B, T, 3072, before its dropout): which side of each ReLU the device took.
// lengths = null: the dense form.  Otherwise B frame counts on the device and their sum (checked by the caller): the ragged form, or, with
// Mp > 0 (xfmr_packed_rows of the same counts), the packed form.
static int xfmr_forward_train_impl(hificar_xfmr* g, const char* what, const float* x, const int* lengths, int valid, float* out, float* bn_batch_stats, int B,
                                   int T, float dropout_p, uint64_t seed, uint64_t offset, void* tape, void* workspace, void* stream_, int Mp = 0) {
    int rc;
    if (!x || !out || !bn_batch_stats) return fail(HIFICAR_E_INVALID, "%s: null tensor", what);
    if (!(dropout_p >= 0.f && dropout_p < 1.f)) return fail(HIFICAR_E_INVALID, "%s: dropout_p=%g outside [0, 1)", what, (double)dropout_p);
    hificar_engine* h = &g->eng;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if ((rc = enter_stream(h, stream)) != HIFICAR_OK) return rc;
    XfmrTrain* ts = g->train;
    if (tape) ts->packed_tapes.erase(tape);  // (the packed entry point records it again once everything is enqueued)
    ts->fwd_precision = g->train_precision;
    const XfmrTrainWs ws = xfmr_plan_train_ws(g, B, T, workspace, Mp);
    const XfmrTape tp = xfmr_plan_tape(g, B, T, tape ? tape : ws.light, Mp);
    const int F = g->cfg.hidden_dim, C = g->cfg.in_channels, O = g->cfg.out_channels, d = F / kXfmrHeads, M = Mp ? Mp : B * T;
    const int* const lens = lengths ? tp.lens : nullptr;
    XfmrTrainCtx cx = {g, h, stream, B, T, M, F, tp.hdr, tp.lens, lens, &ws, {}, {tp.row0, tp.pad_row}};
    auto P = [&](const std::string& name) { return ts->tab.at(name); };
    hipLaunchKernelGGL(bigru_header_kernel, dim3(1), dim3(1), 0, stream, tp.hdr, (unsigned long long)seed, (unsigned long long)offset, dropout_p, B, T,
                       lengths ? valid : M, lengths ? 1 : 0, 1, T, 0);
    HIP_TRY(hipGetLastError());
    if (lengths) HIP_TRY(hipMemcpyAsync(tp.lens, lengths, (size_t)B * sizeof(int), hipMemcpyDeviceToDevice, stream));
    if (Mp) {
        hipLaunchKernelGGL(xfmr_pack_table_kernel, dim3((unsigned)B + 1), dim3(256), 0, stream, tp.lens, B, T, Mp, tp.row0, tp.pad_row);
        HIP_TRY(hipGetLastError());
    }
    // a tap of a ragged forward: the rows of padded frames are zeros (a GEMM's output there is finite, not zero); of a packed forward: the
    // rows go back to the padded (B, T, width) layout, zeros on padded frames
    auto tap = [&](const std::string& name, const float* rows, int width) -> int {
        float* dst;
        const int rc2 = g->taps.find(name, (size_t)(Mp ? B * T : M) * width, &dst);
        if (rc2 != HIFICAR_OK || !dst) return rc2;
        if (Mp) {
            hipLaunchKernelGGL(xfmr_unpack_rows_kernel, dim3((unsigned)std::min<long long>(((long long)T * (width / 4) + 255) / 256, 64), (unsigned)B), dim3(256),
                               0, stream, rows, dst, width, tp.lens, tp.row0, T);
            HIP_TRY(hipGetLastError());
            return HIFICAR_OK;
        }
        HIP_TRY(hipMemcpyAsync(dst, rows, (size_t)M * width * sizeof(float), hipMemcpyDeviceToDevice, stream));
        if (!lengths) return HIFICAR_OK;
        hipLaunchKernelGGL(bigru_zero_pad_kernel, dim3((unsigned)std::min<long long>(((long long)T * (width / 4) + 255) / 256, 8), (unsigned)B), dim3(256), 0,
                           stream, dst, width, tp.lens, T);
        HIP_TRY(hipGetLastError());
        return HIFICAR_OK;
    };
    {
        ProfScope prof(h, stream, "xfmr_rows_kernel", 0.0, 4.0 * M * (C + g->cin_pad));
        hipLaunchKernelGGL(xfmr_rows_kernel, dim3((unsigned)((T + 31) / 32), (unsigned)(g->cin_pad / 32), (unsigned)B), dim3(256), 0, stream, x, tp.xin,
                           lens, C, g->cin_pad, T, tp.row0);
        HIP_TRY(hipGetLastError());
        XT(cx.zero_gaps(tp.xin, g->cin_pad));
    }
    const float* in = tp.xin;
    for (int i = 0; i < 3; ++i) {
        const int j1 = ts->bn_c1[i], j2 = ts->bn_c2[i];
        XfmrTrain::Bn &b1 = ts->bns[(size_t)j1], &b2 = ts->bns[(size_t)j2];
        XT(cx.conv(b1.raw, in, nullptr, tp.y[j1], nullptr));
        XT(cx.bn_stats(tp.y[j1], tp.stats[j1], bn_batch_stats + (size_t)j1 * 2 * F));
        XT(cx.bn_apply(tp.y[j1], tp.stats[j1], P(b1.bn + ".weight"), nullptr, tp.a1[i], true));
        XT(tap("conv_blocks." + std::to_string(i) + ".relu1", tp.a1[i], F));
        XT(cx.conv(b2.raw, tp.a1[i], nullptr, tp.y[j2], nullptr));
        XT(cx.bn_stats(tp.y[j2], tp.stats[j2], bn_batch_stats + (size_t)j2 * 2 * F));
        const float* res = in;
        if (i == 0 && ts->bn_rp >= 0) {
            const int j3 = ts->bn_rp;
            XfmrTrain::Bn& b3 = ts->bns[(size_t)j3];
            XT(cx.conv(b3.raw, in, nullptr, tp.y[j3], nullptr));
            XT(cx.bn_stats(tp.y[j3], tp.stats[j3], bn_batch_stats + (size_t)j3 * 2 * F));
            XT(cx.bn_apply(tp.y[j3], tp.stats[j3], P(b3.bn + ".weight"), nullptr, ws.res, false));
            res = ws.res;
        }
        XT(cx.bn_apply(tp.y[j2], tp.stats[j2], P(b2.bn + ".weight"), res, tp.bo[i], true));
        XT(tap("conv_blocks." + std::to_string(i) + ".relu2", tp.bo[i], F));
        in = tp.bo[i];
    }
    XT(cx.conv(g->w_in, in, nullptr, tp.X[0], nullptr));
    for (int l = 0; l < g->cfg.elayers; ++l) {
        const XfmrEncLayer& E = g->enc[(size_t)l];
        const XfmrTapeLayer& L = tp.L[(size_t)l];
        const float* X = tp.X[(size_t)l];
        XT(cx.conv(E.qkv, X, nullptr, L.qkv, nullptr));
        {
            XfmrAttnParams p;
            p.qkv = L.qkv;
            p.emb = E.d_emb;
            p.lengths = lens;
            p.out = L.o;
            p.T = T;
            p.F = F;
            p.scale = (float)(1.0 / std::sqrt((double)d));
            p.lse = L.lse;
            p.hdr = tp.hdr;
            p.site = 4 * l;
            p.row0 = tp.row0;
            XT(cx.zero_gaps(L.o, F));
            const dim3 grid((unsigned)((T + kXfmrTQ - 1) / kXfmrTQ), kXfmrHeads, (unsigned)B);
            if (xfmr_train_a(g)) {  // bf16x3wa: the same statements on bf16 MFMAs, the tables as xfmr_split_tables left them
                if (!E.d_emb16) return fail(HIFICAR_E_INVALID, "internal: bf16x3wa forward without split position tables");
                const XfmrAttn16TrainParams p16 = {p, xfmr_tab16(E.d_emb16, d)};
                XT(cx.attn("xfmr_attn16_kernel<train>", 2.0 * M * F * 3 * kXfmrTab, 4.0 * M * 4 * F, "xfmr_attn16_train_kernel", d, [&](auto D) {
                    return xfmr_launch(xfmr_attn16_train_kernel<D()>, grid, XfmrAttn16TrainLds<D()>::bytes, stream, p16);
                }));
            } else {
                XT(cx.attn("xfmr_attn_kernel<train>", 2.0 * M * F * 3 * kXfmrTab, 4.0 * M * 4 * F, "xfmr_attn_kernel", d, [&](auto D) {
                    return xfmr_launch(xfmr_attn_kernel<D(), true>, grid, XfmrAttnLds<D()>::bytes, stream, p);
                }));
            }
        }
        XT(cx.conv(E.wo, L.o, nullptr, ws.t1, nullptr));
        XT(cx.add_drop(X, ws.t1, L.p1, 4 * l + 1));
        XT(cx.layer_norm(L.p1, E.d_ln[0], E.d_ln[1], L.n1));
        XT(cx.conv(E.l1, L.n1, nullptr, nullptr, L.hid));
        XT(tap("layers." + std::to_string(l) + ".hidden", L.hid, kXfmrFF));
        XT(cx.gate(nullptr, L.hid, ws.wide, (long long)M * kXfmrFF, 4 * l + 2));
        XT(cx.conv(E.l2, ws.wide, nullptr, ws.t1, nullptr));
        XT(cx.add_drop(L.n1, ws.t1, L.p2, 4 * l + 3));
        XT(cx.layer_norm(L.p2, E.d_ln[2], E.d_ln[3], tp.X[(size_t)l + 1]));
    }
    XT(cx.conv(g->w_out, tp.X[(size_t)g->cfg.elayers], nullptr, ws.wide, nullptr));
    {
        const int Op = g->w_out.cout_pad;
        ProfScope prof(h, stream, "xfmr_out_kernel", 0.0, 4.0 * M * (O + Op));
        hipLaunchKernelGGL(xfmr_out_kernel, dim3((unsigned)((T + 31) / 32), (unsigned)(Op / 32), (unsigned)B), dim3(256), 0, stream, ws.wide, out,
                           lens, O, Op, T, tp.row0);
        HIP_TRY(hipGetLastError());
    }
    return HIFICAR_OK;
}

extern "C" int hificar_xfmr_forward_train(hificar_xfmr* g, const float* x, float* out, float* bn_batch_stats, int B, int T, float dropout_p, uint64_t seed,
                                          uint64_t offset, void* tape, size_t tape_bytes, void* workspace, size_t workspace_bytes, void* stream_) {
    const char* what = "hificar_xfmr_forward_train";
    const int rc = xfmr_train_check(g, what, B, T, tape, tape_bytes, workspace, workspace_bytes, true);
    if (rc != HIFICAR_OK) return rc;
    return xfmr_forward_train_impl(g, what, x, nullptr, B * T, out, bn_batch_stats, B, T, dropout_p, seed, offset, tape, workspace, stream_);
}

// The same step on a ragged batch; see include/hificar.h.  lengths: device int32[B]; lengths_host: the same values on the host (required:
// checked before anything is enqueued).  All lengths = T: every result is bitwise that of hificar_xfmr_forward_train.
extern "C" int hificar_xfmr_forward_train_ragged(hificar_xfmr* g, const float* x, const int32_t* lengths, const int32_t* lengths_host, float* out,
                                                 float* bn_batch_stats, int B, int T, float dropout_p, uint64_t seed, uint64_t offset, void* tape,
                                                 size_t tape_bytes, void* workspace, size_t workspace_bytes, void* stream_) {
    const char* what = "hificar_xfmr_forward_train_ragged";
    // the arguments first (they need no device), then the handle's state
    if (!g) return fail(HIFICAR_E_INVALID, "%s: null handle", what);
    if (B < 1 || T < 1) return fail(HIFICAR_E_INVALID, "%s: B=%d, T=%d out of range", what, B, T);
    if (!lengths || !lengths_host) return fail(HIFICAR_E_INVALID, "%s: lengths and lengths_host are both required", what);
    long long valid = 0;
    for (int b = 0; b < B; ++b) {
        if (lengths_host[b] < 0 || lengths_host[b] > T) return fail(HIFICAR_E_INVALID, "%s: lengths[%d]=%d outside [0, %d]", what, b, (int)lengths_host[b], T);
        valid += lengths_host[b];
    }
    if (valid < 2) return fail(HIFICAR_E_INVALID, "%s: batch statistics need more than one valid frame (sum of lengths = %lld)", what, valid);
    const int rc = xfmr_train_check(g, what, B, T, tape, tape_bytes, workspace, workspace_bytes, true);
    if (rc != HIFICAR_OK) return rc;
    return xfmr_forward_train_impl(g, what, x, lengths, (int)valid, out, bn_batch_stats, B, T, dropout_p, seed, offset, tape, workspace, stream_);
}

// The same step on a packed batch; see include/hificar.h.  The rows of every buffer are the Mp packed rows (XfmrLayout); the user-facing
// tensors keep the padded layout.
extern "C" int hificar_xfmr_forward_train_packed(hificar_xfmr* g, const float* x, const int32_t* lengths, const int32_t* lengths_host, float* out,
                                                 float* bn_batch_stats, int B, int T, float dropout_p, uint64_t seed, uint64_t offset, void* tape,
                                                 size_t tape_bytes, void* workspace, size_t workspace_bytes, void* stream_) {
    const char* what = "hificar_xfmr_forward_train_packed";
    if (!g) return fail(HIFICAR_E_INVALID, "%s: null handle", what);
    if (B < 1 || T < 1) return fail(HIFICAR_E_INVALID, "%s: B=%d, T=%d out of range", what, B, T);
    if (!lengths || !lengths_host) return fail(HIFICAR_E_INVALID, "%s: lengths and lengths_host are both required", what);
    for (int b = 0; b < B; ++b)
        if (lengths_host[b] < 0 || lengths_host[b] > T) return fail(HIFICAR_E_INVALID, "%s: lengths[%d]=%d outside [0, %d]", what, b, (int)lengths_host[b], T);
    long long valid = 0;
    const long long mp = xfmr_packed_rows(B, T, lengths_host, &valid);
    if (valid < 2) return fail(HIFICAR_E_INVALID, "%s: batch statistics need more than one valid frame (sum of lengths = %lld)", what, valid);
    if (mp * kXfmrFF >= (1LL << 31)) return fail(HIFICAR_E_INVALID, "%s: %lld packed rows out of range (packed rows * 3072 < 2^31)", what, mp);
    int rc = xfmr_train_check(g, what, B, T, tape, tape_bytes, workspace, workspace_bytes, true, (int)mp);
    if (rc != HIFICAR_OK) return rc;
    rc = xfmr_forward_train_impl(g, what, x, lengths, (int)valid, out, bn_batch_stats, B, T, dropout_p, seed, offset, tape, workspace, stream_, (int)mp);
    if (rc == HIFICAR_OK && tape) g->train->packed_tapes[tape] = {B, T, std::vector<int32_t>(lengths_host, lengths_host + B)};
    return rc;
}

static int xfmr_backward_impl(hificar_xfmr* g, const float* dout, int B, int T, int Mp, const void* tape, float* grads, float* dx, void* workspace,
                              void* stream_);

// A tape goes back through the arithmetic that filled it: the handle remembers its last training forward's (no device read-back)
static int xfmr_backward_arith(const hificar_xfmr* g, const char* what) {
    if (g->train->fwd_precision == g->train_precision) return HIFICAR_OK;
    return fail(HIFICAR_E_STATE, "%s: the handle's training arithmetic is %s, its last training forward ran in %s (hificar_xfmr_set_train_precision between "
                                 "a forward and its backward)", what, xfmr_precision_name(g->train_precision), xfmr_precision_name(g->train->fwd_precision));
}

extern "C" int hificar_xfmr_backward(hificar_xfmr* g, const float* dout, int B, int T, const void* tape, size_t tape_bytes, float* grads, float* dx,
                                     void* workspace, size_t workspace_bytes, void* stream_) {
    const char* what = "hificar_xfmr_backward";
    if (g && g->train && g->train->packed_tapes.count(tape))  // (first: a packed tape is sized by other rows)
        return fail(HIFICAR_E_STATE, "%s: this tape was filled by hificar_xfmr_forward_train_packed; its backward is hificar_xfmr_backward_packed", what);
    int rc = xfmr_train_check(g, what, B, T, const_cast<void*>(tape), tape_bytes, workspace, workspace_bytes);
    if (rc != HIFICAR_OK) return rc;
    if (!dout || !grads) return fail(HIFICAR_E_INVALID, "%s: null tensor", what);
    if ((rc = xfmr_backward_arith(g, what)) != HIFICAR_OK) return rc;
    return xfmr_backward_impl(g, dout, B, T, 0, tape, grads, dx, workspace, stream_);
}

// The backward of a packed tape; see include/hificar.h.  lengths_host: the forward's frame counts, which give Mp on the host; they are
// checked against what the handle recorded when it filled the tape.
extern "C" int hificar_xfmr_backward_packed(hificar_xfmr* g, const float* dout, const int32_t* lengths_host, int B, int T, const void* tape,
                                            size_t tape_bytes, float* grads, float* dx, void* workspace, size_t workspace_bytes, void* stream_) {
    const char* what = "hificar_xfmr_backward_packed";
    if (!g) return fail(HIFICAR_E_INVALID, "%s: null handle", what);
    if (!lengths_host) return fail(HIFICAR_E_INVALID, "%s: lengths_host is required", what);
    const int mp = hificar_xfmr_packed_rows(B, T, lengths_host);
    if (!mp) return fail(HIFICAR_E_INVALID, "%s: B=%d, T=%d and these lengths are no packed batch (each length in 0 .. T, their sum >= 2)", what, B, T);
    int rc = xfmr_train_init(g);
    if (rc != HIFICAR_OK) return rc;
    const auto it = g->train->packed_tapes.find(tape);
    if (it == g->train->packed_tapes.end())
        return fail(HIFICAR_E_STATE, "%s: this tape was not filled by hificar_xfmr_forward_train_packed on this handle (a dense or ragged tape's backward "
                                     "is hificar_xfmr_backward)", what);
    if (it->second.B != B || it->second.T != T || !std::equal(it->second.lengths.begin(), it->second.lengths.end(), lengths_host))
        return fail(HIFICAR_E_INVALID, "%s: B, T or the lengths differ from those of the forward that filled this tape", what);
    rc = xfmr_train_check(g, what, B, T, const_cast<void*>(tape), tape_bytes, workspace, workspace_bytes, false, mp);
    if (rc != HIFICAR_OK) return rc;
    if (!dout || !grads) return fail(HIFICAR_E_INVALID, "%s: null tensor", what);
    if ((rc = xfmr_backward_arith(g, what)) != HIFICAR_OK) return rc;
    return xfmr_backward_impl(g, dout, B, T, mp, tape, grads, dx, workspace, stream_);
}

// Both backwards, checked by their entry points.  Mp = 0: a dense or ragged tape; otherwise a packed one of Mp rows.
static int xfmr_backward_impl(hificar_xfmr* g, const float* dout, int B, int T, int Mp, const void* tape, float* grads, float* dx, void* workspace,
                              void* stream_) {
    int rc;
    hificar_engine* h = &g->eng;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if ((rc = enter_stream(h, stream)) != HIFICAR_OK) return rc;
    XfmrTrain* ts = g->train;
    const XfmrTape tp = xfmr_plan_tape(g, B, T, const_cast<void*>(tape), Mp);
    const XfmrTrainWs ws = xfmr_plan_train_ws(g, B, T, workspace, Mp);
    const int F = g->cfg.hidden_dim, C = g->cfg.in_channels, O = g->cfg.out_channels, d = F / kXfmrHeads, M = Mp ? Mp : B * T, FF = kXfmrFF;
    XfmrTrainCtx cx = {g, h, stream, B, T, M, F, tp.hdr, tp.lens, nullptr, &ws, {}, {tp.row0, tp.pad_row}};
    cx.bw.partial = ws.partial;
    cx.bw.colsum = ws.colsum;
    cx.bw.partial_elems = ws.partial_elems;
    cx.bw.colsum_elems = ws.colsum_elems;
    cx.bw.accumulate = false;
    cx.bw.defer = nullptr;
    auto P = [&](const std::string& name) { return ts->tab.at(name); };
    auto G = [&](const std::string& name) { return grads + ts->tab.offset.at(name); };
    const long long MF = (long long)M * F;
    float *d0 = ws.d[0], *d1 = ws.d[1], *d2 = ws.d[2];
    const int E = g->cfg.elayers, Op = g->w_out.cout_pad;
    {   // dout (B, O, T) -> rows [B T][Op]; a ragged tape: dout past a length is not read, its rows are zeros
        ProfScope prof(h, stream, "xfmr_rows_kernel", 0.0, 4.0 * M * (O + Op));
        hipLaunchKernelGGL(xfmr_drows_kernel, dim3((unsigned)((T + 31) / 32), (unsigned)(Op / 32), (unsigned)B), dim3(256), 0, stream, dout, ws.wide, tp.hdr,
                           tp.lens, O, Op, T, cx.lay);
        HIP_TRY(hipGetLastError());
        XT(cx.zero_gaps(ws.wide, Op));
    }
    XT(cx.wgrad(g->w_out, ws.wide, Op, tp.X[(size_t)E], F, G("w_out.weight"), G("w_out.bias")));
    XT(cx.conv(ts->dg_wout, ws.wide, nullptr, d0, nullptr, false));
    for (int l = E - 1; l >= 0; --l) {
        const std::string b = "transformer.layers." + std::to_string(l) + ".";
        const XfmrEncLayer& L = g->enc[(size_t)l];
        const XfmrTrainLayer& D = ts->enc[(size_t)l];
        const XfmrTapeLayer& K = tp.L[(size_t)l];
        // norm2, the join n1 + dropout2(linear2(...))
        XT(cx.ln_bwd(K.p2, d0, L.d_ln[2], G(b + "norm2.weight"), d1));                 // d1 = d p2 (= the residual's share of d n1)
        XT(cx.gate(nullptr, d1, d2, MF, 4 * l + 3));                                   // d2 = d linear2's output
        XT(cx.gate(nullptr, K.hid, ws.wide, (long long)M * FF, 4 * l + 2));            // linear2's input, as the forward made it
        XT(cx.wgrad(L.l2, d2, F, ws.wide, FF, G(b + "linear2.weight"), G(b + "linear2.bias")));
        XT(cx.conv(D.dg_l2, d2, nullptr, ws.gw, nullptr, false));
        XT(cx.gate(K.hid, ws.gw, ws.gw, (long long)M * FF, 4 * l + 2));                // through the dropout and the ReLU
        XT(cx.wgrad(L.l1, ws.gw, FF, K.n1, F, G(b + "linear1.weight"), G(b + "linear1.bias")));
        XT(cx.conv(D.dg_l1, ws.gw, d1, d2, nullptr, false));                           // d2 = d n1
        // norm1, the join x + dropout1(w_o(attention))
        XT(cx.ln_bwd(K.p1, d2, L.d_ln[0], G(b + "norm1.weight"), d1));                 // d1 = d p1 (= the residual's share of d x)
        XT(cx.gate(nullptr, d1, d2, MF, 4 * l + 1));                                   // d2 = d w_o's output
        XT(cx.wgrad(L.wo, d2, F, K.o, F, ts->d_wscr, nullptr));
        hipLaunchKernelGGL(transpose_kernel, dim3(1024), dim3(256), 0, stream, ts->d_wscr, G(b + "self_attn.w_o"), F, F);
        HIP_TRY(hipGetLastError());
        XT(cx.conv(D.dg_wo, d2, nullptr, d0, nullptr, false));                         // d0 = d O
        {
            XfmrAttnBwdParams p;
            p.qkv = K.qkv;
            p.emb = L.d_emb;
            p.o = K.o;
            p.dout = d0;
            p.lse = K.lse;
            p.dqkv = ws.gw;
            p.ds = ws.ds;
            p.pd = ws.pd;
            p.hdr = tp.hdr;
            p.lens = tp.lens;
            p.site = 4 * l;
            p.T = T;
            p.F = F;
            p.scale = (float)(1.0 / std::sqrt((double)d));
            p.lay = cx.lay;
            XT(cx.zero_gaps(ws.gw, 3 * F));
            const int chunks = (M + kXfmrEmbRows - 1) / kXfmrEmbRows;
            const dim3 grid((unsigned)((T + kXfmrTQ - 1) / kXfmrTQ), kXfmrHeads, (unsigned)B);
            if (xfmr_train_a(g)) {  // bf16x3wa: S, dPd and both parts of dQ on bf16 MFMAs; dK, dV, dE in the fp32 kernels, on the same banded buffers
                if (!L.d_emb16) return fail(HIFICAR_E_INVALID, "internal: bf16x3wa backward without split position tables");
                const XfmrAttn16BwdParams p16 = {p, xfmr_tab16(L.d_emb16, d)};
                XT(cx.attn("xfmr_attn16_bwd_q_kernel", 2.0 * M * F * 4 * kXfmrTab, 4.0 * M * (6.0 * F + 2.0 * kXfmrHeads * kXfmrBand), "xfmr_attn16_bwd_q_kernel", d,
                           [&](auto D) { return xfmr_launch(xfmr_attn16_bwd_q_kernel<D()>, grid, XfmrAttn16TrainLds<D()>::bytes, stream, p16); }));
                if (xfmr_train_k(g)) {  // bf16x3wack: dK, dV and dE's first stage on bf16 MFMAs too, from the same banded buffers
                    XT(cx.attn("xfmr_attn16_bwd_k_kernel", 2.0 * M * F * 2 * kXfmrTab, 4.0 * M * (4.0 * F + 2.0 * kXfmrHeads * kXfmrBand), "xfmr_attn16_bwd_k_kernel",
                               d, [&](auto D) { return xfmr_launch(xfmr_attn16_bwd_k_kernel<D()>, grid, XfmrAttn16BwdKLds<D()>::bytes, stream, p); }));
                    XT(cx.attn("xfmr_demb16_partial_kernel", 2.0 * M * F * kXfmrTab, 4.0 * M * (1.0 * F + 1.0 * kXfmrHeads * kXfmrBand), "xfmr_demb16_partial_kernel",
                               d, [&](auto D) {
                                   return xfmr_launch(xfmr_demb16_partial_kernel<D()>, dim3((unsigned)chunks, kXfmrHeads), XfmrEmb16Lds<D()>::bytes, stream, p.qkv, p.ds,
                                                      ws.embpart, M, p.T, p.F, p.hdr, p.lens, p.lay);
                               }));
                } else {
                    XT(cx.attn("xfmr_attn_bwd_k_kernels", 2.0 * M * F * 3 * kXfmrTab, 4.0 * M * (5.0 * F + 3.0 * kXfmrHeads * kXfmrBand), "attention backward", d,
                               [&](auto D) { return xfmr_attn_bwd_k_launch<D()>(p, grid, ws.embpart, M, chunks, stream); }));
                }
            } else {
                // S, dP, dQ (K and E parts), dK, dV, dE: six banded products of 2 M F 199 flops each
                XT(cx.attn("xfmr_attn_bwd_kernels", 2.0 * M * F * 7 * kXfmrTab, 4.0 * M * (8.0 * F + 4.0 * kXfmrHeads * kXfmrBand), "attention backward", d,
                           [&](auto D) { return xfmr_attn_bwd_launch<D()>(p, grid, ws.embpart, M, chunks, stream); }));
            }
            const int width = kXfmrHeads * kXfmrTab * d;
            hipLaunchKernelGGL(bigru_colreduce_kernel, dim3((unsigned)((width + 255) / 256)), dim3(256), 0, stream, ws.embpart, chunks, width,
                               G(b + "self_attn.relative_positional.embeddings"));
            HIP_TRY(hipGetLastError());
        }
        XT(cx.wgrad(L.qkv, ws.gw, 3 * F, tp.X[(size_t)l], F, ts->d_wscr, nullptr));
        hipLaunchKernelGGL(xfmr_qkv_weight_kernel, dim3(1024), dim3(256), 0, stream, G(b + "self_attn.w_q"), G(b + "self_attn.w_k"), G(b + "self_attn.w_v"),
                           ts->d_wscr, F, d, 1);
        HIP_TRY(hipGetLastError());
        XT(cx.conv(D.dg_qkv, ws.gw, d1, d0, nullptr, false));                          // d0 = d x: the layer below's output gradient
    }
    XT(cx.wgrad(g->w_in, d0, F, tp.bo[2], F, G("w_raw_in.weight"), G("w_raw_in.bias")));
    XT(cx.conv(ts->dg_win, d0, nullptr, d1, nullptr, false));                          // d1 = d (the last ResBlock's output)
    for (int i = 2; i >= 0; --i) {
        const int j1 = ts->bn_c1[i], j2 = ts->bn_c2[i];
        XfmrTrain::Bn &b1 = ts->bns[(size_t)j1], &b2 = ts->bns[(size_t)j2];
        const float* in = i ? tp.bo[i - 1] : tp.xin;
        const int in_pitch = i ? F : g->cin_pad;
        XT(cx.gate(tp.bo[i], d1, d1, MF, -1));                                          // d1 = dz: through the block's last ReLU
        XT(cx.bn_bwd(tp.y[j2], d1, tp.stats[j2], P(b2.bn + ".weight"), G(b2.bn + ".weight"), d2));
        XT(cx.wgrad(b2.raw, d2, F, tp.a1[i], F, G(b2.conv + ".weight"), G(b2.conv + ".bias"), &b2.wg3));
        XT(cx.conv(b2.dg, d2, nullptr, d0, nullptr));
        XT(cx.gate(tp.a1[i], d0, d0, MF, -1));
        XT(cx.bn_bwd(tp.y[j1], d0, tp.stats[j1], P(b1.bn + ".weight"), G(b1.bn + ".weight"), d0));
        XT(cx.wgrad(b1.raw, d0, F, in, in_pitch, G(b1.conv + ".weight"), G(b1.conv + ".bias"), &b1.wg3));
        if (i > 0) {
            XT(cx.conv(b1.dg, d0, d1, d2, nullptr));                                    // + the identity residual's dz
            std::swap(d1, d2);
            continue;
        }
        const float* dres = d1;  // the residual path's share of d (input rows): dz itself without a residual_path (then cin_pad = F)
        if (ts->bn_rp >= 0) {
            XfmrTrain::Bn& b3 = ts->bns[(size_t)ts->bn_rp];
            XT(cx.bn_bwd(tp.y[ts->bn_rp], d1, tp.stats[ts->bn_rp], P(b3.bn + ".weight"), G(b3.bn + ".weight"), d2));
            XT(cx.wgrad(b3.raw, d2, F, tp.xin, g->cin_pad, G(b3.conv + ".weight"), G(b3.conv + ".bias")));
            if (dx) XT(cx.conv(b3.dg, d2, nullptr, ws.dxr[0], nullptr));
            dres = ws.dxr[0];
        }
        if (dx) {
            XT(cx.conv(b1.dg, d0, dres, ws.dxr[1], nullptr));
            ProfScope prof(h, stream, "xfmr_unrows_kernel", 0.0, 4.0 * M * (C + g->cin_pad));
            hipLaunchKernelGGL(xfmr_unrows_kernel, dim3((unsigned)((T + 31) / 32), (unsigned)(g->cin_pad / 32), (unsigned)B), dim3(256), 0, stream, ws.dxr[1], dx,
                               tp.hdr, tp.lens, C, g->cin_pad, T, cx.lay);
            HIP_TRY(hipGetLastError());
        }
    }
    return HIFICAR_OK;
}
#undef XT

// Test aid: the bf16 fragments of a Conv1d weight w (cout, cin, K; host floats; input rows cin_pad wide) as the bf16x3 training arithmetic
// builds them.  mode 0: the layer's own pack; 2: its data gradient's.  how 0: pack16_kernel's index functions run on the host (no device);
// 1: pack16_kernel itself, over a buffer of 0xFF bytes; 2: pack_w16, the host pack of the inference handles, read back from the device.
// out: `capacity` bf16 elements; *elems: how many the pack has (the zero tail included).
extern "C" int hificar_debug_pack16(int cout, int cin, int cin_pad, int K, int mode, int how, const float* w, uint16_t* out, size_t capacity, size_t* elems) {
    if (!w || !out || !elems || (mode != 0 && mode != 2) || how < 0 || how > 2 || K < 1 || K % 2 != 1) return fail(HIFICAR_E_INVALID, "hificar_debug_pack16: bad argument");
    ConvLayer P;
    int rc = mode == 0 ? xfmr_plan(P, "debug", cin, cin_pad, cout, K) : xfmr_plan(P, "debug#dgrad", cout, round_up(cout, 32), cin, K);
    if (rc != HIFICAR_OK) return rc;
    const size_t n = xfmr_pack16_bytes(P) / sizeof(uint16_t);
    *elems = n;
    if (capacity < n) return fail(HIFICAR_E_INVALID, "hificar_debug_pack16: %zu elements, the buffer has %zu", n, capacity);
    const size_t wn = (size_t)cout * cin * K;
    if (how == 0) {
        memset(out, 0xFF, n * sizeof(uint16_t));
        const Pack16Params p = xfmr_pack16_params(P, w, out, mode, cin, cout);
        for (long long i = 0; i < pack16_items(p); ++i) pack16_item(p, i);
        memset(out + pack16_frags(p) * 512, 0, (size_t)4 * p.nc16 * 512 * sizeof(uint16_t));
        return HIFICAR_OK;
    }
    if (how == 1) {
        void *dw = nullptr, *dp = nullptr;
        HIP_TRY(hipMalloc(&dw, wn * sizeof(float)));
        hipError_t e = hipMalloc(&dp, n * sizeof(uint16_t));
        if (e == hipSuccess) e = hipMemcpy(dw, w, wn * sizeof(float), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemset(dp, 0xFF, n * sizeof(uint16_t));
        if (e == hipSuccess) {
            const Pack16Params p = xfmr_pack16_params(P, static_cast<const float*>(dw), static_cast<uint16_t*>(dp), mode, cin, cout);
            hipLaunchKernelGGL(pack16_kernel, dim3((unsigned)std::min<long long>((pack16_items(p) + 255) / 256, 2048)), dim3(256), 0, nullptr, p);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpy(out, dp, n * sizeof(uint16_t), hipMemcpyDeviceToHost);
        (void)hipFree(dw);
        (void)hipFree(dp);
        HIP_TRY(e);
        return HIFICAR_OK;
    }
    HostTensor W;
    W.shape = {P.cout, P.cin, K};
    W.data.resize(wn);
    for (int co = 0; co < P.cout; ++co)
        for (int ci = 0; ci < P.cin; ++ci)
            for (int t = 0; t < K; ++t)
                W.data[((size_t)co * P.cin + ci) * K + t] = mode == 0 ? w[((size_t)co * cin + ci) * K + t] : w[((size_t)ci * cin + co) * K + (K - 1 - t)];
    hificar_engine tmp;
    uint16_t* d = nullptr;
    rc = pack_w16(&tmp, P, W, P.chunk16, &d);
    hipError_t e = rc == HIFICAR_OK ? hipMemcpy(out, d, n * sizeof(uint16_t), hipMemcpyDeviceToHost) : hipSuccess;
    for (void* p : tmp.allocs) (void)hipFree(p);
    if (rc != HIFICAR_OK) return rc;
    HIP_TRY(e);
    return HIFICAR_OK;
}

// Test aid: the split of fp32 rows x [M][C] (host floats) into 8-row groups, as the bf16x3w training arithmetic's weight gradients read them
// (xfmr_split_rows_t_kernel).  lengths / T (B = M / T sequences; null: dense) mark a ragged batch's padded frames, pad_row (M entries, < 0: a
// gap row; null: none) a packed batch's gap rows; both kinds of row are written as zero bits.  how 0: the kernel's index functions run on the
// host (no device); 1: the kernel itself, over a buffer of 0xFF bytes.  out: `capacity` bytes; *bytes: how many the split has.
extern "C" int hificar_debug_split_rows_t(int M, int C, int T, const int32_t* lengths, const int32_t* pad_row, int how, const float* x, void* out,
                                          size_t capacity, size_t* bytes) {
    if (!x || !out || !bytes || M < 1 || C < 1 || how < 0 || how > 1 || (long long)M * C >= (1LL << 31) || (lengths && (T < 1 || M % T)) || (lengths && pad_row))
        return fail(HIFICAR_E_INVALID, "hificar_debug_split_rows_t: bad argument");
    const size_t n = (size_t)split_t_bytes(M, C);
    *bytes = n;
    if (capacity < n) return fail(HIFICAR_E_INVALID, "hificar_debug_split_rows_t: %zu bytes, the buffer has %zu", n, capacity);
    if (how == 0) {
        memset(out, 0xFF, n);
        auto valid = [&](long long r) { return pad_row ? pad_row[r] >= 0 : !lengths || r % T < std::min(std::max(lengths[r / T], 0), T); };
        for (long long i = 0; i < split_t_items(M, C); ++i) split_t_item(x, static_cast<char*>(out), M, C, i, valid);
        return HIFICAR_OK;
    }
    void *dx = nullptr, *dd = nullptr, *dl = nullptr;
    const int32_t* table = pad_row ? pad_row : lengths;
    const size_t tn = pad_row ? (size_t)M : lengths ? (size_t)(M / T) : 0;
    hipError_t e = hipMalloc(&dx, (size_t)M * C * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&dd, n);
    if (e == hipSuccess && tn) e = hipMalloc(&dl, tn * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpy(dx, x, (size_t)M * C * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess && tn) e = hipMemcpy(dl, table, tn * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dd, 0xFF, n);
    if (e == hipSuccess) {
        XfmrLayout lay;
        if (pad_row) lay.pad_row = static_cast<const int*>(dl);
        hipLaunchKernelGGL(xfmr_split_rows_t_kernel, dim3((unsigned)std::min<long long>((split_t_items(M, C) + 255) / 256, 8192)), dim3(256), 0, nullptr,
                           static_cast<const float*>(dx), static_cast<char*>(dd), (long long)M, C, nullptr, pad_row ? nullptr : static_cast<const int*>(dl),
                           T > 0 ? T : 1, lay);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, dd, n, hipMemcpyDeviceToHost);
    (void)hipFree(dx);
    (void)hipFree(dd);
    (void)hipFree(dl);
    HIP_TRY(e);
    return HIFICAR_OK;
}

// Test aid: the tap-column split of fp32 rows x [M][C] (host floats) into 8-row groups of 3 C columns, as the bf16x3wac training arithmetic's
// k = 3 weight gradients read their A operand (xfmr_split_taps_t_kernel): column k C + c of row r is row r + k - 1 of channel c, zero bits
// where that row is outside [0, M), a padded frame, a gap row or another sequence's.  T > 0: M / T sequences of T rows (lengths: their frame
// counts; null: dense); T = 0 (lengths null): one sequence of M rows.  pad_row (M entries, < 0: a gap row): a packed batch, T is not used.
// how 0: the kernel's index functions run on the host (no device); 1: the kernel itself, over a buffer of 0xFF bytes.  out: `capacity`
// bytes; *bytes: how many the split has.
extern "C" int hificar_debug_split_taps_t(int M, int C, int T, const int32_t* lengths, const int32_t* pad_row, int how, const float* x, void* out,
                                          size_t capacity, size_t* bytes) {
    if (!x || !out || !bytes || M < 1 || C < 1 || T < 0 || how < 0 || how > 1 || (long long)M * C * 3 >= (1LL << 31) || (T > 0 && M % T) || (lengths && T < 1) ||
        (lengths && pad_row))
        return fail(HIFICAR_E_INVALID, "hificar_debug_split_taps_t: bad argument");
    const size_t n = (size_t)split_t3_bytes(M, C);
    *bytes = n;
    if (capacity < n) return fail(HIFICAR_E_INVALID, "hificar_debug_split_taps_t: %zu bytes, the buffer has %zu", n, capacity);
    const int Ts = T > 0 ? T : M;
    if (how == 0) {
        memset(out, 0xFF, n);
        auto valid = [&](long long r) { return pad_row ? pad_row[r] >= 0 : !lengths || r % Ts < std::min(std::max(lengths[r / Ts], 0), Ts); };
        for (long long i = 0; i < split_t3_items(M, C); ++i) split_t3_item(x, static_cast<char*>(out), M, C, pad_row ? (long long)M + 8 : (long long)Ts, i, valid);
        return HIFICAR_OK;
    }
    void *dx = nullptr, *dd = nullptr, *dl = nullptr;
    const int32_t* table = pad_row ? pad_row : lengths;
    const size_t tn = pad_row ? (size_t)M : lengths ? (size_t)(M / Ts) : 0;
    hipError_t e = hipMalloc(&dx, (size_t)M * C * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&dd, n);
    if (e == hipSuccess && tn) e = hipMalloc(&dl, tn * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpy(dx, x, (size_t)M * C * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess && tn) e = hipMemcpy(dl, table, tn * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dd, 0xFF, n);
    if (e == hipSuccess) {
        XfmrLayout lay;
        if (pad_row) lay.pad_row = static_cast<const int*>(dl);
        hipLaunchKernelGGL(xfmr_split_taps_t_kernel, dim3((unsigned)std::min<long long>((split_t3_items(M, C) + 255) / 256, 8192)), dim3(256), 0, nullptr,
                           static_cast<const float*>(dx), static_cast<char*>(dd), (long long)M, C, nullptr, pad_row ? nullptr : static_cast<const int*>(dl), Ts, lay);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, dd, n, hipMemcpyDeviceToHost);
    (void)hipFree(dx);
    (void)hipFree(dd);
    (void)hipFree(dl);
    HIP_TRY(e);
    return HIFICAR_OK;
}
