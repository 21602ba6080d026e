// Discriminator side of libhificar (included at the end of hificar.hip): HiFiGANMultiScaleMultiPeriodDiscriminator forward and backward
// for the reference's train step (articulatory/bin/train.py:340-440; articulatory/models/hifigan.py:317-825).  Every Conv1d /
// Conv2d (k, 1) is an im2col gather (hificar_disc_kernels.hip.h) + ONE GEMM per group on the generator's exact-fp32 conv kernels
// (a single-tap ConvLayer: cin = k * cin_g im2col columns); the data gradient is the same kernel on the transposed pack, the weight
// gradient the all-taps wgrad kernel with one tap.  Exact fp32.

struct DiscGroup {
    ConvLayer F;  // forward GEMM: cin = Kg, cout = cout_g
    ConvLayer D;  // data gradient GEMM: cin = cout_g, cout = Kg_pad
    // sliding-window layers (long sequences: the scale discriminators' strided grouped layers) in the POLYPHASE-INPUT form: the zero-padded
    // activations X [seq][Lp][cin_g] read as rows of `stride` positions are a (stride * cin_g)-channel sequence, and the strided conv is a
    // plain ceil(k / stride)-tap stride-1 conv over it: out[t] = sum_q W'[q] . X4[t + q], W'[q][r * cin_g + c] = W[c][stride * q + r] — the
    // shape the conv kernels are built for (an LDS item = taps x K slabs instead of one 32-column slice of an im2col row per barrier)
    ConvLayer P;  // forward: cin' = stride * cin_g -> cout_g, taps 0 .. ntaps - 1 (padding 0)
    ConvLayer Q;  // data gradient: cout_g -> cin', a Conv1d with padding ntaps - 1 over dZ, writes dX4 (= dX at padded positions)
    int co0 = 0, ci0 = 0;
};

struct DiscLayer {
    std::string base;  // state_dict prefix of the conv ("msd.discriminators.0.layers.1.0")
    int cin = 0, cout = 0, k = 0, stride = 1, pad = 0, groups = 1;
    bool act = true, has_bias = true, conv2d = false;
    int cin_g = 0, cout_g = 0, Kg = 0, Kg_pad = 0, Np = 0;
    bool can_window = false;  // a Conv1d on previous-layer channels whose strided data gradient fits the polyphase conv kernel
    std::vector<DiscGroup> g;
};

struct DiscSub {
    int period = 0;  // 0: scale discriminator
    int scale = 0;   // pooling level of a scale discriminator
    float slope = 0.1f;
    std::vector<DiscLayer> layers;
};

struct hificar_disc {
    hificar_disc_config cfg;
    bool col2im_vec4 = true;  // HIFICAR_COL2IM_VEC4=0: the scalar col2im_mask_kernel everywhere (A/B runs)
    hificar_engine eng;
    std::vector<DiscSub> subs;
    // folded parameters in state_dict order; gradient buckets: one per sub-discriminator (its parameters are contiguous, raw and folded alike)
    RawParamSet raw;
    bool grad_accumulate = false;        // hificar_disc_set_grad_accumulate
    const float* grad_scale = nullptr;   // hificar_disc_set_grad_scale
    // the sub-discriminators are independent networks of small launches: each runs on its own stream between a fork and a join on the
    // caller's stream (HIFICAR_DISC_STREAMS=0: everything on the caller's stream)
    bool use_streams = true;
    int n_side = 8;           // side streams; sub si runs on side[sub_stream[si] % n_side]
    std::vector<int> sub_stream;
    bool use_windows = true;  // false: im2col for every layer
    int window_min_rows = 32; // sequences at least this long take the window form 
    std::vector<hipStream_t> side;
    std::vector<hipEvent_t> join_ev;
    hipEvent_t fork_ev = nullptr;
    // loss tables (hificar_disc_loss), one per (B, T, mode, configuration)
    struct LossTable {
        LossEntry* d_entries = nullptr;
        int n = 0;
        std::vector<int> out_index;  // entry -> output buffer index
    };
    std::map<std::string, LossTable> loss_tables;
};

static int disc_fork(hificar_disc* d, hipStream_t main) {
    if (!d->use_streams) return HIFICAR_OK;
    if (d->side.empty()) {
        HIP_TRY(hipEventCreateWithFlags(&d->fork_ev, hipEventDisableTiming));
        const size_t ns = std::max<size_t>(1, std::min<size_t>(d->subs.size(), (size_t)d->n_side));
        d->side.resize(ns);
        d->join_ev.resize(ns);
        for (size_t i = 0; i < ns; ++i) {
            HIP_TRY(hipStreamCreateWithFlags(&d->side[i], hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&d->join_ev[i], hipEventDisableTiming));
        }
    }
    HIP_TRY(hipEventRecord(d->fork_ev, main));
    for (hipStream_t s : d->side) HIP_TRY(hipStreamWaitEvent(s, d->fork_ev, 0));
    return HIFICAR_OK;
}

static int disc_join(hificar_disc* d, hipStream_t main) {
    if (!d->use_streams) return HIFICAR_OK;
    for (size_t i = 0; i < d->side.size(); ++i) {
        HIP_TRY(hipEventRecord(d->join_ev[i], d->side[i]));
        HIP_TRY(hipStreamWaitEvent(main, d->join_ev[i], 0));
    }
    return HIFICAR_OK;
}

// (an input shorter than the kernel has no output position: 0, not the 1 that C's division towards zero would make of it)
static int disc_out_len(int L, int k, int stride, int pad) { return L + 2 * pad < k ? 0 : (L + 2 * pad - k) / stride + 1; }

struct DiscGeom {
    int nseq = 0;
    int T_sub = 0;       // signal length this sub-discriminator reads (scale: the pooled length; period: T)
    std::vector<int> L;  // L[0] rows per sequence of the input, L[l + 1] of layer l's output
};

static DiscGeom disc_geom(const hificar_disc* d, const DiscSub& s, int B, int T) {
    DiscGeom g;
    if (s.period == 0) {
        int t = T;
        for (int i = 0; i < s.scale; ++i) t = disc_out_len(t, d->cfg.pool_kernel, d->cfg.pool_stride, d->cfg.pool_pad);
        g.nseq = B;
        g.T_sub = t;
        g.L.push_back(t);
    } else {
        g.nseq = B * s.period;
        g.T_sub = T;
        g.L.push_back((T + s.period - 1) / s.period);
    }
    for (const DiscLayer& L : s.layers) g.L.push_back(disc_out_len(g.L.back(), L.k, L.stride, L.pad));
    return g;
}

// Buffers of one (B, T) call: the tape (im2col matrices A and layer outputs Y of every group; the pooled signals) and, for the backward,
// dZ / dA of every group, the pooled signals' gradients and the weight-gradient partials.
struct DiscPlan {
    struct LayerBuf {
        size_t A = 0, Y = 0;          // offsets (floats) of group 0; group g at + g * a_stride / y_stride
        size_t a_stride = 0, y_stride = 0;
        long long M = 0;
        // sliding-window form (long sequences of the scale discriminators): the tape holds the padded activations X [group][seq][Lp][cin_g]
        // instead of the im2col matrix; the GEMM stages its rows as overlapping windows of X (ConvParams::x_row_bytes)
        int Lp = 0;  // > 0: sliding-window form, time steps per sequence of X
    };
    std::vector<std::vector<LayerBuf>> tape;  // [sub][layer]
    std::vector<size_t> pooled;               // [scale] offset of the pooled signal (scale 0: the input itself, unused)
    size_t tape_floats = 0;
    std::vector<std::vector<LayerBuf>> bwd;   // same shape: A -> dA, Y -> dZ
    std::vector<size_t> dpooled;              // [scale >= 1] gradient of the pooled signal (sum target of the pool chain)
    std::vector<size_t> dsig;                 // [sub] gradient of that sub-discriminator's own input signal (B x T_sub)
    std::vector<size_t> partial, colsum;      // [sub] weight-gradient partial sums / bias column sums
    std::vector<size_t> partial_elems, colsum_elems;
    size_t ws_floats = 0;
    std::vector<DiscGeom> geom;
};

static DiscPlan disc_plan(const hificar_disc* d, int B, int T) {
    DiscPlan p;
    Carver tape(nullptr, 1024), ws(nullptr, 1024);  // (offsets in floats into the caller's tape and backward workspace)
    int n_scales = 0;
    for (const DiscSub& s : d->subs)
        if (s.period == 0) n_scales = std::max(n_scales, s.scale + 1);
    p.pooled.assign((size_t)n_scales, 0);
    p.dpooled.assign((size_t)n_scales, 0);
    for (const DiscSub& s : d->subs) {
        size_t pe = 0, ce = 0;
        const DiscGeom g = disc_geom(d, s, B, T);
        p.geom.push_back(g);
        if (s.period == 0 && s.scale > 0) {
            p.pooled[(size_t)s.scale] = tape.floats_at((size_t)B * g.T_sub);
            p.dpooled[(size_t)s.scale] = ws.floats_at((size_t)B * g.T_sub);
        }
        std::vector<DiscPlan::LayerBuf> tl, bl;
        for (size_t l = 0; l < s.layers.size(); ++l) {
            const DiscLayer& L = s.layers[l];
            DiscPlan::LayerBuf t, b;
            t.M = b.M = (long long)g.nseq * g.L[l + 1];
            t.a_stride = b.a_stride = round_up_sz((size_t)t.M * L.Kg_pad * sizeof(float), 1024) / sizeof(float);
            if (d->use_windows && L.can_window && s.layers[l - 1].cout_g % 4 == 0 && g.L[l + 1] >= d->window_min_rows) {
                // X [group][seq][Lp][cin_g], Lp = stride * (L_out + ntaps - 1) positions = L_out + ntaps - 1 rows of the polyphase-input conv
                // (it covers the left padding + the data: stride * L_out >= L_in + 2 pad - k + 1 and stride * (ntaps - 1) >= k - stride)
                t.Lp = b.Lp = L.stride * (g.L[l + 1] + L.g[0].P.ntaps - 1);
                t.a_stride = round_up_sz((size_t)g.nseq * t.Lp * L.cin_g * sizeof(float), 1024) / sizeof(float);
                b.a_stride = t.a_stride;  // backward: dX at the same padded positions
            }
            t.y_stride = b.y_stride = round_up_sz((size_t)t.M * L.Np * sizeof(float), 1024) / sizeof(float);
            t.A = tape.floats_at(t.a_stride * L.groups);
            t.Y = tape.floats_at(t.y_stride * L.groups);
            b.A = ws.floats_at(b.a_stride * L.groups);
            b.Y = ws.floats_at(b.y_stride * L.groups);
            tl.push_back(t);
            bl.push_back(b);
            // (every layer its own piece of the scratch: the sub-discriminator's reductions run as one launch at the end of its pass)
            pe += (size_t)L.groups * (t.Lp ? wgrad_partial_elems(&d->eng, L.g[0].P, g.nseq, g.L[l + 1]) : wgrad_partial_elems(&d->eng, L.g[0].F, 1, (int)t.M));
            ce += (size_t)L.groups * (t.Lp ? wgrad_colsum_elems(&d->eng, L.g[0].P, g.nseq, g.L[l + 1]) : wgrad_colsum_elems(&d->eng, L.g[0].F, 1, (int)t.M));
        }
        p.tape.push_back(tl);
        p.bwd.push_back(bl);
        p.dsig.push_back(ws.floats_at((size_t)B * g.T_sub));
        p.partial_elems.push_back(pe);
        p.partial.push_back(ws.floats_at(pe));
        p.colsum_elems.push_back(ce);
        p.colsum.push_back(ws.floats_at(ce));
    }
    p.tape_floats = tape.bytes() / sizeof(float);
    p.ws_floats = ws.bytes() / sizeof(float);
    return p;
}

static int disc_add_layer(hificar_disc* d, DiscSub& s, const std::string& base, int cin, int cout, int k, int stride, int pad, int groups,
                          bool act, bool has_bias, bool conv2d) {
    if (cin < 1 || cout < 1 || k < 1 || stride < 1 || pad < 0 || groups < 1 || cin % groups || cout % groups)
        return fail(HIFICAR_E_INVALID, "discriminator layer %s: bad shape (cin %d cout %d k %d stride %d groups %d)", base.c_str(), cin, cout, k,
                    stride, groups);
    DiscLayer L;
    L.base = base;
    L.cin = cin;
    L.cout = cout;
    L.k = k;
    L.stride = stride;
    L.pad = pad;
    L.groups = groups;
    L.act = act;
    L.has_bias = has_bias;
    L.conv2d = conv2d;
    L.cin_g = cin / groups;
    L.cout_g = cout / groups;
    L.Kg = L.cin_g * k;
    L.Kg_pad = round_up(L.Kg, 32);
    L.Np = round_up(L.cout_g, 32);
    L.g.resize((size_t)groups);
    hificar_engine* h = &d->eng;
    for (int gi = 0; gi < groups; ++gi) {
        DiscGroup& G = L.g[(size_t)gi];
        G.co0 = gi * L.cout_g;
        G.ci0 = gi * L.cin_g;
        ConvLayer& F = G.F;
        F = ConvLayer();
        F.name = base + "#g" + std::to_string(gi);
        F.cin = L.Kg;
        F.cin_pad = L.Kg_pad;
        F.cout = L.cout_g;
        F.K = 1;
        F.dilation = 1;
        F.padding = 0;
        F.has_bias = true;
        int rc = plan_layer(F);
        if (rc != HIFICAR_OK) return rc;
        ConvLayer& D = G.D;
        D = ConvLayer();
        D.name = F.name + "#dgrad";
        D.cin = L.cout_g;
        D.cin_pad = L.Np;
        D.cout = L.Kg_pad;
        D.K = 1;
        D.dilation = 1;
        D.padding = 0;
        D.has_bias = false;
        if ((rc = plan_layer(D)) != HIFICAR_OK) return rc;
    }
    const int ntaps_p = (k + stride - 1) / stride;
    L.can_window = !conv2d && !s.layers.empty() && k > 1 && L.cin_g % 4 == 0 && (stride * L.cin_g) % 32 == 0 && ntaps_p >= 2 && ntaps_p <= 11;
    if (L.can_window)
        for (int gi = 0; gi < groups; ++gi) {
            ConvLayer& P = L.g[(size_t)gi].P;
            P = ConvLayer();
            P.name = base + "#g" + std::to_string(gi) + "#poly";
            P.cin = P.cin_pad = stride * L.cin_g;
            P.cout = L.cout_g;
            P.K = ntaps_p;
            P.dilation = 1;
            P.padding = 0;
            P.has_bias = true;
            int rc = plan_layer(P);
            if (rc != HIFICAR_OK) return rc;
            ConvLayer& Q = L.g[(size_t)gi].Q;
            Q = ConvLayer();
            Q.name = base + "#g" + std::to_string(gi) + "#polydgrad";
            Q.cin = L.cout_g;
            Q.cin_pad = L.Np;
            Q.cout = stride * L.cin_g;
            Q.K = ntaps_p;
            Q.dilation = 1;
            Q.padding = ntaps_p - 1;
            Q.has_bias = false;
            if ((rc = plan_layer(Q)) != HIFICAR_OK) return rc;
        }
    // the groups' packs and biases lie at regular strides (one launch covers every group: ConvRep)
    for (int which = 0; which < (L.can_window ? 4 : 2); ++which) {
        ConvLayer& P0 = which == 3 ? L.g[0].Q : which == 2 ? L.g[0].P : which ? L.g[0].D : L.g[0].F;
        const size_t pe = pack_w32_elems(P0, P0.chunk16), be = (size_t)P0.cout_total;
        void* p = nullptr;
        HIP_TRY(hipMalloc(&p, pe * groups * sizeof(float)));
        h->allocs.push_back(p);
        HIP_TRY(hipMemset(p, 0, pe * groups * sizeof(float)));
        float* wbase = static_cast<float*>(p);
        HIP_TRY(hipMalloc(&p, be * groups * sizeof(float)));
        h->allocs.push_back(p);
        HIP_TRY(hipMemset(p, 0, be * groups * sizeof(float)));
        float* bbase = static_cast<float*>(p);
        for (int gi = 0; gi < groups; ++gi) {
            ConvLayer& P = which == 3 ? L.g[(size_t)gi].Q : which == 2 ? L.g[(size_t)gi].P : which ? L.g[(size_t)gi].D : L.g[(size_t)gi].F;
            P.d_w32 = wbase + (size_t)gi * pe;
            P.d_bias = bbase + (size_t)gi * be;
        }
    }
    auto slot = [&](const std::string& name, const std::vector<int64_t>& shape) { d->raw.add(name, shape, (int)d->subs.size()); };
    // state_dict order: a weight-normed Conv2d lists bias first (bias, weight_g, weight_v); a plain Conv1d weight, bias
    if (conv2d) {
        slot(base + ".bias", {cout});
        slot(base + ".weight", {cout, L.cin_g, k, 1});
    } else {
        slot(base + ".weight", {cout, L.cin_g, k});
        if (has_bias) slot(base + ".bias", {cout});
    }
    s.layers.push_back(L);
    return HIFICAR_OK;
}

extern "C" int hificar_disc_create(const hificar_disc_config* cfg, hificar_disc** out) {
    if (!cfg || !out) return fail(HIFICAR_E_INVALID, "hificar_disc_create: null argument");
    const hificar_disc_config& c = *cfg;
    if (c.n_scales < 0 || c.n_scales > HIFICAR_DISC_MAX_SUBS || c.n_periods < 0 || c.n_periods > HIFICAR_DISC_MAX_SUBS || c.n_scales + c.n_periods < 1)
        return fail(HIFICAR_E_INVALID, "discriminator: %d scales / %d periods out of range", c.n_scales, c.n_periods);
    if (c.s_n_layers > HIFICAR_DISC_MAX_LAYERS || c.p_n_layers > HIFICAR_DISC_MAX_LAYERS || (c.n_scales && c.s_n_layers < 2) ||
        (c.n_periods && c.p_n_layers < 2))
        return fail(HIFICAR_E_INVALID, "discriminator: layer count out of range");
    if (c.n_scales > 1 && (c.pool_kernel < 1 || c.pool_stride < 1 || c.pool_pad < 0 || 2 * c.pool_pad > c.pool_kernel))
        return fail(HIFICAR_E_INVALID, "discriminator: bad AvgPool1d parameters");
    hificar_disc* d = new hificar_disc();
    d->cfg = c;
    hificar_engine* h = &d->eng;
    int rc = engine_open(h, true);
    h->precision = HIFICAR_PREC_F32;
    h->use_pair = false;
    // HIFICAR_DISC_STREAMS=0: every sub-discriminator on the caller's stream (launches do not overlap: per-launch counters, tools/collect_profiles.sh);
    // the tile shapes stay those of the overlapped run.  HIFICAR_COL2IM_VEC4=0: the scalar gathers (bit-identity test).
    if (const char* e = getenv("HIFICAR_DISC_STREAMS")) d->use_streams = atoi(e) != 0;
    if (const char* e = getenv("HIFICAR_COL2IM_VEC4")) d->col2im_vec4 = atoi(e) != 0;
    h->pick_throughput = 64;
    h->mi1_penalty = 1.3;
    if (rc == HIFICAR_OK) rc = wgrad_setup();
    auto bail = [&](int code) {
        engine_close(h);
        delete d;
        return code;
    };
    if (rc != HIFICAR_OK) return bail(rc);
    for (int i = 0; i < c.n_scales; ++i) {
        DiscSub s;
        s.period = 0;
        s.scale = i;
        s.slope = c.s_slope;
        for (int l = 0; l < c.s_n_layers; ++l) {
            const bool act = l + 1 < c.s_n_layers;
            const std::string base = "msd.discriminators." + std::to_string(i) + ".layers." + std::to_string(l) + (act ? ".0" : "");
            if ((rc = disc_add_layer(d, s, base, c.s_cin[l], c.s_cout[l], c.s_k[l], c.s_stride[l], c.s_pad[l], c.s_groups[l], act, c.s_bias != 0,
                                     false)) != HIFICAR_OK)
                return bail(rc);
        }
        d->subs.push_back(s);
    }
    for (int i = 0; i < c.n_periods; ++i) {
        if (c.periods[i] < 1) return bail(fail(HIFICAR_E_INVALID, "discriminator: period %d", c.periods[i]));
        DiscSub s;
        s.period = c.periods[i];
        s.slope = c.p_slope;
        for (int l = 0; l < c.p_n_layers; ++l) {
            const bool act = l + 1 < c.p_n_layers;
            const std::string base = "mpd.discriminators." + std::to_string(i) + (act ? ".convs." + std::to_string(l) + ".0" : ".output_conv");
            if ((rc = disc_add_layer(d, s, base, c.p_cin[l], c.p_cout[l], c.p_k[l], c.p_stride[l], c.p_pad[l], 1, act, true, true)) != HIFICAR_OK)
                return bail(rc);
        }
        d->subs.push_back(s);
    }
    d->raw.n_buckets = (int)d->subs.size();
    for (size_t j = 1; j < d->raw.slots.size(); ++j)  // (hificar_disc_bucket_folded_range and the job order rely on it)
        if (d->raw.slots[j].bucket < d->raw.slots[j - 1].bucket)
            return bail(fail(HIFICAR_E_INVALID, "internal: sub-discriminator parameters are not contiguous"));
    d->sub_stream.resize(d->subs.size());
    for (size_t i = 0; i < d->subs.size(); ++i) d->sub_stream[i] = (int)i;
    *out = d;
    return HIFICAR_OK;
}

extern "C" void hificar_disc_destroy(hificar_disc* d) {
    if (!d) return;
    for (hipStream_t s : d->side) (void)hipStreamDestroy(s);
    for (hipEvent_t e : d->join_ev) (void)hipEventDestroy(e);
    if (d->fork_ev) (void)hipEventDestroy(d->fork_ev);
    engine_close(&d->eng);
    delete d;
}

extern "C" hificar_engine* hificar_disc_engine(hificar_disc* d) { return d ? &d->eng : nullptr; }
extern "C" int hificar_disc_param_count(const hificar_disc* d) { return d ? (int)d->raw.slots.size() : -1; }

extern "C" int hificar_disc_param_info(const hificar_disc* d, int i, char* name96, int64_t* shape4, int* ndim, int64_t* offset) {
    if (!d || i < 0 || i >= (int)d->raw.slots.size() || !name96) return fail(HIFICAR_E_INVALID, "hificar_disc_param_info: bad argument");
    const auto& s = d->raw.slots[(size_t)i];
    snprintf(name96, 96, "%s", s.name.c_str());
    if (shape4)
        for (size_t k = 0; k < 4; ++k) shape4[k] = k < s.shape.size() ? s.shape[k] : 1;
    if (ndim) *ndim = (int)s.shape.size();
    if (offset) *offset = s.offset;
    return HIFICAR_OK;
}

extern "C" int64_t hificar_disc_grad_floats(const hificar_disc* d) { return d ? d->raw.total : -1; }
extern "C" int64_t hificar_disc_raw_grad_floats(const hificar_disc* d) { return d && d->raw.have_params ? d->raw.raw_total : -1; }

// Every pack of the discriminators (forward + data gradient of each group's GEMM, modes 8-11), its sources inside the master copy.
static int disc_pack_jobs(const hificar_disc* d, std::vector<PackParams>& jobs) {
    for (const DiscSub& s : d->subs)
        for (const DiscLayer& L : s.layers) {
            const float* w = d->raw.d_folded + d->raw.offset(L.base + ".weight");
            const float* b = L.has_bias ? d->raw.d_folded + d->raw.offset(L.base + ".bias") : nullptr;
            for (const DiscGroup& G : L.g) {
                PackParams pp;
                fill_pack(pp, G.F, G.F.chunk16);
                pp.src = w + (size_t)G.co0 * L.cin_g * L.k;
                pp.dst = G.F.d_w32;
                pp.mode = 8;
                pp.cin = L.cin_g;
                pp.K = L.k;
                pp.cout = L.cout_g;
                pp.cout_pack = L.cout_g;
                pp.cin_pack = L.Kg;
                jobs.push_back(pp);
                fill_pack(pp, G.D, G.D.chunk16);
                pp.src = w + (size_t)G.co0 * L.cin_g * L.k;
                pp.dst = G.D.d_w32;
                pp.mode = 9;
                pp.cin = L.cin_g;
                pp.K = L.k;
                pp.cout = L.cout_g;
                pp.cout_pack = L.Kg;
                pp.cin_pack = L.cout_g;
                jobs.push_back(pp);
                if (L.can_window) {  // polyphase-input form: the forward pack (mode 10) and its data gradient's (mode 11)
                    fill_pack(pp, G.P, G.P.chunk16);
                    pp.src = w + (size_t)G.co0 * L.cin_g * L.k;
                    pp.dst = G.P.d_w32;
                    pp.mode = 10;
                    pp.cin = L.cin_g;
                    pp.K = L.k;
                    pp.cout = L.cout_g;
                    pp.stride = L.stride;
                    pp.cout_pack = L.cout_g;
                    pp.cin_pack = L.stride * L.cin_g;
                    jobs.push_back(pp);
                    fill_pack(pp, G.Q, G.Q.chunk16);
                    pp.src = w + (size_t)G.co0 * L.cin_g * L.k;
                    pp.dst = G.Q.d_w32;
                    pp.mode = 11;
                    pp.cin = L.cin_g;
                    pp.K = L.k;
                    pp.cout = L.cout_g;
                    pp.stride = L.stride;
                    pp.cout_pack = L.stride * L.cin_g;
                    pp.cin_pack = L.cout_g;
                    jobs.push_back(pp);
                    if (b) jobs.push_back(simple_pack(7, b + G.co0, G.P.d_bias, L.cout_g));
                }
                if (b) jobs.push_back(simple_pack(7, b + G.co0, G.F.d_bias, L.cout_g));
            }
        }
    return HIFICAR_OK;
}

// Every parameter in its RAW state_dict form from device memory (weight_g / weight_v of the weight-normed period discriminators, plain
// weights of the scale discriminators — hifigan.py:645-663 never norms those —, biases): weight norm folded on the device into a master
// copy, every GEMM pack (forward + data gradient) refreshed from it.  Two launches.  Same contract as hificar_set_parameters_device.
extern "C" int hificar_disc_set_parameters_device(hificar_disc* d, const char* const* names, const float* const* data, int n, void* stream_) {
    if (!d || !names || !data || n < 1) return fail(HIFICAR_E_INVALID, "hificar_disc_set_parameters_device: null argument");
    return raw_set_parameters(&d->eng, d->raw, "hificar_disc_set_parameters_device", names, data, n, static_cast<hipStream_t>(stream_),
                              [d](std::vector<PackParams>& jobs) { return disc_pack_jobs(d, jobs); });
}

extern "C" int hificar_disc_weight_norm_backward(hificar_disc* d, const float* grads, float* raw_grads, void* stream_) {
    if (!d || !grads || !raw_grads) return fail(HIFICAR_E_INVALID, "hificar_disc_weight_norm_backward: null argument");
    if (!d->raw.have_params) return fail(HIFICAR_E_STATE, "hificar_disc_weight_norm_backward needs hificar_disc_set_parameters_device first");
    return raw_weight_norm_backward(&d->eng, d->raw, grads, raw_grads, -1, d->grad_scale, static_cast<hipStream_t>(stream_));
}

// Two switches for the criterion's backward (include/hificar.h): the second pass of a discriminator update adds its parameter gradients
// to the first pass's buffer (no second buffer, no add pass), and the weight-norm chain rule multiplies by the upstream gradient of the
// scalar loss while it writes (no scaling pass).
extern "C" int hificar_disc_set_grad_accumulate(hificar_disc* d, int on) {
    if (!d) return fail(HIFICAR_E_INVALID, "hificar_disc_set_grad_accumulate: null handle");
    d->grad_accumulate = on != 0;
    return HIFICAR_OK;
}

extern "C" int hificar_disc_set_grad_scale(hificar_disc* d, const float* scale_device) {
    if (!d) return fail(HIFICAR_E_INVALID, "hificar_disc_set_grad_scale: null handle");
    d->grad_scale = scale_device;
    return HIFICAR_OK;
}

// ---- gradient buckets: one per sub-discriminator (include/hificar.h: "data-parallel training") ----
extern "C" int hificar_disc_grad_bucket_count(const hificar_disc* d) { return d ? (int)d->subs.size() : -1; }

extern "C" int hificar_disc_raw_param_bucket(const hificar_disc* d, int i) { return raw_param_bucket(d ? &d->raw : nullptr, i); }

// the bucket's slice of the FOLDED gradient buffer (hificar_disc_backward's `grads`): floats [*offset, *offset + *numel)
extern "C" int hificar_disc_bucket_folded_range(const hificar_disc* d, int bucket, int64_t* offset, int64_t* numel) {
    if (!d || !offset || !numel || !d->raw.have_params || bucket < 0 || bucket >= (int)d->subs.size())
        return fail(HIFICAR_E_INVALID, "hificar_disc_bucket_folded_range: bad argument (or no parameters handed over yet)");
    const RawParamSet& r = d->raw;
    const int lo = r.bucket_job_lo[(size_t)bucket], hi = r.bucket_job_lo[(size_t)bucket + 1];
    *offset = lo < (int)r.slots.size() ? r.slots[(size_t)lo].offset : r.total;
    *numel = (hi < (int)r.slots.size() ? r.slots[(size_t)hi].offset : r.total) - *offset;
    return HIFICAR_OK;
}

extern "C" int hificar_disc_set_bucket_callback(hificar_disc* d, hificar_bucket_fn fn, void* user) {
    if (!d) return fail(HIFICAR_E_INVALID, "null handle");
    d->raw.bucket_fn = fn;
    d->raw.bucket_user = user;
    return HIFICAR_OK;
}

// hificar_disc_weight_norm_backward for ONE sub-discriminator; called from the bucket callback on the stream it hands over.
extern "C" int hificar_disc_weight_norm_backward_bucket(hificar_disc* d, const float* grads, float* raw_grads, int bucket, void* stream_) {
    if (!d || !grads || !raw_grads) return fail(HIFICAR_E_INVALID, "hificar_disc_weight_norm_backward_bucket: null argument");
    if (!d->raw.have_params) return fail(HIFICAR_E_STATE, "hificar_disc_weight_norm_backward_bucket needs hificar_disc_set_parameters_device first");
    if (bucket < 0 || bucket >= d->raw.n_buckets) return fail(HIFICAR_E_INVALID, "bucket %d out of range", bucket);
    return raw_weight_norm_backward(&d->eng, d->raw, grads, raw_grads, bucket, d->grad_scale, static_cast<hipStream_t>(stream_));
}

extern "C" size_t hificar_disc_tape_bytes(const hificar_disc* d, int B, int T) {
    if (!d || B < 1 || T < 2) return 0;
    return disc_plan(d, B, T).tape_floats * sizeof(float);
}

// Algorithmic multiply-accumulates of ONE forward pass over (B, 1, T): sum over every conv of (output positions) x cout x (cin / groups) x k
// (bias / activation / pooling excluded) — the discriminators' counterpart of hificar_macs, for bench.py's training roofline.
extern "C" double hificar_disc_macs(const hificar_disc* d, int B, int T) {
    if (!d || B < 1 || T < 2) return 0.0;
    double macs = 0.0;
    for (const DiscSub& s : d->subs) {
        const DiscGeom g = disc_geom(d, s, B, T);
        for (size_t l = 0; l < s.layers.size(); ++l) {
            const DiscLayer& L = s.layers[l];
            macs += (double)g.nseq * std::max(g.L[l + 1], 0) * L.cout * L.cin_g * L.k;
        }
    }
    return macs;
}

extern "C" size_t hificar_disc_backward_workspace_bytes(const hificar_disc* d, int B, int T) {
    if (!d || B < 1 || T < 2) return 0;
    return disc_plan(d, B, T).ws_floats * sizeof(float);
}

// Output buffers (one per sub-discriminator, layer and group), in forward order.
extern "C" int hificar_disc_output_count(const hificar_disc* d) {
    if (!d) return -1;
    int n = 0;
    for (const DiscSub& s : d->subs)
        for (const DiscLayer& L : s.layers) n += L.groups;
    return n;
}

extern "C" int hificar_disc_output_info(const hificar_disc* d, int B, int T, int i, hificar_disc_output* out) {
    if (!d || !out || B < 1 || T < 2 || i < 0) return fail(HIFICAR_E_INVALID, "hificar_disc_output_info: bad argument");
    const DiscPlan p = disc_plan(d, B, T);
    int n = 0;
    for (size_t si = 0; si < d->subs.size(); ++si)
        for (size_t l = 0; l < d->subs[si].layers.size(); ++l) {
            const DiscLayer& L = d->subs[si].layers[l];
            if (i < n + L.groups) {
                const int gi = i - n;
                out->sub = (int)si;
                out->layer = (int)l;
                out->group = gi;
                out->n_groups = L.groups;
                out->period = d->subs[si].period;
                out->offset_bytes = (int64_t)((p.tape[si][l].Y + (size_t)gi * p.tape[si][l].y_stride) * sizeof(float));
                out->nseq = p.geom[si].nseq;
                out->rows = p.geom[si].L[l + 1];
                out->pitch = L.Np;
                out->channels = L.cout_g;
                return HIFICAR_OK;
            }
            n += L.groups;
        }
    return fail(HIFICAR_E_INVALID, "hificar_disc_output_info: index %d out of range", i);
}

static unsigned ew_blocks(const hificar_engine* h, long long n) { return (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, 16LL * h->num_cus)); }

// x (B, 1, T) -> every layer output of every sub-discriminator, kept in `tape` (hificar_disc_output_info locates them).
extern "C" int hificar_disc_forward(hificar_disc* d, const float* x, int B, int T, void* tape_, size_t tape_bytes, void* stream_) {
    if (!d || !x || !tape_) return fail(HIFICAR_E_INVALID, "hificar_disc_forward: null argument");
    if (!d->raw.have_params) return fail(HIFICAR_E_STATE, "hificar_disc_forward needs hificar_disc_set_parameters_device first");
    if (B < 1 || T < 2) return fail(HIFICAR_E_INVALID, "hificar_disc_forward: B=%d T=%d", B, T);
    for (const DiscSub& s : d->subs)
        if (s.period > 0 && (s.period - T % s.period) % s.period >= T)
            return fail(HIFICAR_E_INVALID, "reflect padding needs T > the pad (period %d, T %d)", s.period, T);
    const DiscPlan p = disc_plan(d, B, T);
    // (checked before anything is enqueued, the pool chain included, and before the fork: an error return must not leave the side streams forked)
    for (size_t si = 0; si < d->subs.size(); ++si)
        for (size_t l = 0; l < d->subs[si].layers.size(); ++l)
            if (p.tape[si][l].M < 1) return fail(HIFICAR_E_INVALID, "discriminator: T=%d is too short for %s", T, d->subs[si].layers[l].base.c_str());
    if (tape_bytes < p.tape_floats * sizeof(float)) return fail(HIFICAR_E_WORKSPACE, "discriminator tape too small: %zu < %zu", tape_bytes, p.tape_floats * sizeof(float));
    if (reinterpret_cast<uintptr_t>(tape_) % 256) return fail(HIFICAR_E_INVALID, "discriminator tape must be 256-byte aligned");
    hificar_engine* h = &d->eng;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    int rc;
    if ((rc = enter_stream(h, stream)) != HIFICAR_OK) return rc;
    float* tape = static_cast<float*>(tape_);
    const Ragged rg;
    hipStream_t main_stream = stream;
    // the AvgPool1d chain of the scale discriminators' inputs (hifigan.py:736-738), on the caller's stream before the fork
    for (size_t si = 0; si < d->subs.size(); ++si) {
        const DiscSub& s = d->subs[si];
        if (s.period != 0 || s.scale == 0) continue;
        const DiscGeom& g = p.geom[si];
        const float* prev = s.scale == 1 ? x : tape + p.pooled[(size_t)s.scale - 1];
        int Lp = T;
        for (int i = 0; i + 1 < s.scale; ++i) Lp = disc_out_len(Lp, d->cfg.pool_kernel, d->cfg.pool_stride, d->cfg.pool_pad);
        PoolParams pp;
        pp.src = prev;
        pp.dst = tape + p.pooled[(size_t)s.scale];
        pp.L_src = Lp;
        pp.L_dst = g.T_sub;
        pp.total = (long long)B * g.T_sub;
        pp.kernel = d->cfg.pool_kernel;
        pp.stride = d->cfg.pool_stride;
        pp.pad = d->cfg.pool_pad;
        pp.accumulate = 0;
        ProfScope prof(h, stream, "avgpool_kernel", 0.0, 8.0 * pp.total);
        hipLaunchKernelGGL(avgpool_kernel, dim3(ew_blocks(h, pp.total)), dim3(256), 0, stream, pp);
        HIP_TRY(hipGetLastError());
    }
    if ((rc = disc_fork(d, main_stream)) != HIFICAR_OK) return rc;
    // (the forked region runs inside a lambda so that EVERY error return below still joins the side streams: the caller's stream must never be
    // left waiting on — or racing with — work that was enqueued on them before the failure)
    rc = [&]() -> int {
    for (size_t si = 0; si < d->subs.size(); ++si) {
        const DiscSub& s = d->subs[si];
        const DiscGeom& g = p.geom[si];
        if (d->use_streams) stream = d->side[(size_t)d->sub_stream[si] % d->side.size()];
        const float* sig = (s.period == 0 && s.scale > 0) ? tape + p.pooled[(size_t)s.scale] : x;
        for (size_t l = 0; l < s.layers.size(); ++l) {
            const DiscLayer& L = s.layers[l];
            const DiscPlan::LayerBuf& tb = p.tape[si][l];
            {
                Im2colParams ip;
                memset(&ip, 0, sizeof(ip));
                ip.dst = tape + tb.A;
                ip.dst_gstride = (long long)tb.a_stride;
                ip.per_group4 = tb.M * (L.Kg_pad / 4);
                ip.total4 = ip.per_group4 * L.groups;
                ip.Kg = L.Kg;
                ip.Kg_pad = L.Kg_pad;
                ip.L_in = g.L[l];
                ip.L_out = g.L[l + 1];
                ip.kt = L.k;
                ip.stride = L.stride;
                ip.pad = L.pad;
                ip.cin_g = L.cin_g;
                if (tb.Lp) {  // X[group][seq][tp][c] = in[seq][tp - pad][group * cin_g + c], zeros outside: a one-tap gather
                    ip.per_group4 = (long long)g.nseq * tb.Lp * (L.cin_g / 4);
                    ip.total4 = ip.per_group4 * L.groups;
                    ip.Kg = ip.Kg_pad = L.cin_g;
                    ip.L_out = tb.Lp;
                    ip.kt = 1;
                    ip.stride = 1;
                }
                ip.T = g.T_sub;
                ip.period = s.period;
                if (l == 0) {
                    ip.src = sig;
                    ip.src_mode = s.period ? 1 : 0;
                    ip.prev_cout_g = 1;
                } else {
                    const DiscLayer& P = s.layers[l - 1];
                    ip.src = tape + p.tape[si][l - 1].Y;
                    ip.src_mode = 2;
                    ip.prev_cout_g = P.cout_g;
                    ip.prev_np = P.Np;
                    ip.prev_gstride = (long long)p.tape[si][l - 1].y_stride;
                }
                const bool vec4 = d->col2im_vec4 && ip.src_mode == 2 && ip.cin_g % 4 == 0 && ip.prev_cout_g % 4 == 0 && ip.prev_np % 4 == 0 &&
                                  ip.prev_gstride % 4 == 0 && ip.dst_gstride % 4 == 0 && ip.per_group4 < (1LL << 31) && L.groups <= 65535 &&
                                  (reinterpret_cast<uintptr_t>(ip.src) | reinterpret_cast<uintptr_t>(ip.dst)) % 16 == 0;
                // (with profile_detail the row says which gather ran: " v4" the 4-wide kernel, " v1" the scalar one — the conv rows' " xN" convention)
                ProfScope prof(h, stream, h->profile_detail ? "im2col_kernel|" + L.base + (vec4 ? " v4" : " v1") : std::string("im2col_kernel"), 0.0,
                               8.0 * tb.M * L.Kg_pad * L.groups);
                if (vec4) hipLaunchKernelGGL(im2col4_kernel, dim3(ew_blocks(h, ip.per_group4), (unsigned)L.groups), dim3(256), 0, stream, ip);
                else hipLaunchKernelGGL(im2col_kernel, dim3(ew_blocks(h, ip.total4)), dim3(256), 0, stream, ip);
                HIP_TRY(hipGetLastError());
            }
            {
                const ConvLayer& FL = tb.Lp ? L.g[0].P : L.g[0].F;
                ConvIO io{};
                float* y = tape + tb.Y;
                io.xs = reinterpret_cast<const char*>(tape + tb.A);
                io.y = L.act ? nullptr : y;
                io.ys = L.act ? reinterpret_cast<char*>(y) : nullptr;
                if (tb.Lp) {  // rows of `stride` padded positions; every row of X exists (the gather zero-filled the padding)
                    io.x_seq_bytes = (long long)tb.Lp * L.cin_g * 4;
                    io.x_rows = tb.Lp / L.stride;
                }
                ConvRep zr;
                zr.n = L.groups;
                zr.zs_x = (long long)tb.a_stride * 4;
                zr.zs_y = (long long)tb.y_stride;
                zr.zs_w = (long long)pack_w32_elems(FL, FL.chunk16) * 4;
                zr.zs_b = FL.cout_total;
                if ((rc = tb.Lp ? launch_conv1(h, FL, g.nseq, g.L[l + 1], io, s.slope, rg, stream, zr)
                                : launch_conv1(h, FL, 1, (int)tb.M, io, s.slope, rg, stream, zr)) != HIFICAR_OK)
                    return rc;
            }
        }
    }
    return HIFICAR_OK;
    }();
    {
        const int rcj = disc_join(d, main_stream);
        return rc != HIFICAR_OK ? rc : rcj;
    }
}

// Gradients of one hificar_disc_forward.  douts[i]: gradient of output buffer i (hificar_disc_output_info order; same [nseq][rows][pitch]
// layout, padded columns ignored) or NULL for zero.  grads: folded-parameter gradients (hificar_disc_grad_floats floats, slot offsets
// from hificar_disc_param_info) or NULL when only the signal gradient is wanted (the generator's adversarial / feature-matching step,
// train.py:341-362).  dx: (B, T) gradient of the input signal or NULL.
extern "C" int hificar_disc_backward(hificar_disc* d, const float* const* douts, int B, int T, const void* tape_, size_t tape_bytes, float* grads,
                                     float* dx, void* ws_, size_t ws_bytes, void* stream_) {
    if (!d || !douts || !tape_ || !ws_) return fail(HIFICAR_E_INVALID, "hificar_disc_backward: null argument");
    if (!d->raw.have_params) return fail(HIFICAR_E_STATE, "hificar_disc_backward needs hificar_disc_set_parameters_device first");
    const DiscPlan p = disc_plan(d, B, T);
    if (tape_bytes < p.tape_floats * sizeof(float) || ws_bytes < p.ws_floats * sizeof(float))
        return fail(HIFICAR_E_WORKSPACE, "discriminator backward: tape / workspace too small");
    if (reinterpret_cast<uintptr_t>(ws_) % 256) return fail(HIFICAR_E_INVALID, "discriminator workspace must be 256-byte aligned");
    hificar_engine* h = &d->eng;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    int rc;
    if ((rc = enter_stream(h, stream)) != HIFICAR_OK) return rc;
    const float* tape = static_cast<const float*>(tape_);
    float* ws = static_cast<float*>(ws_);
    const Ragged rg;
    hipStream_t main_stream = stream;
    // output buffer index of (sub, layer, group 0)
    std::vector<std::vector<int>> obase(d->subs.size());
    {
        int n = 0;
        for (size_t si = 0; si < d->subs.size(); ++si)
            for (const DiscLayer& L : d->subs[si].layers) {
                obase[si].push_back(n);
                n += L.groups;
            }
    }
    int n_scales = 0;
    for (const DiscSub& s : d->subs)
        if (s.period == 0) n_scales = std::max(n_scales, s.scale + 1);
    if ((rc = disc_fork(d, main_stream)) != HIFICAR_OK) return rc;
    // (the forked region runs inside a lambda so that EVERY error return below still joins the side streams: the caller's stream must never be
    // left waiting on — or racing with — work that was enqueued on them before the failure)
    rc = [&]() -> int {
    for (size_t si = 0; si < d->subs.size(); ++si) {
        const DiscSub& s = d->subs[si];
        const DiscGeom& g = p.geom[si];
        const int nl = (int)s.layers.size();
        if (d->use_streams) stream = d->side[(size_t)d->sub_stream[si] % d->side.size()];
        BwdWs bw;
        memset(&bw, 0, sizeof(bw));
        bw.partial = ws + p.partial[si];
        bw.partial_elems = p.partial_elems[si];
        bw.colsum = ws + p.colsum[si];
        bw.colsum_elems = p.colsum_elems[si];
        DeferredReduce pending;
        bw.defer = &pending;
        bw.accumulate = d->grad_accumulate;
        for (int l = nl - 1; l >= 0; --l) {
            const DiscLayer& L = s.layers[(size_t)l];
            const DiscPlan::LayerBuf& tb = p.tape[si][(size_t)l];
            const DiscPlan::LayerBuf& bb = p.bwd[si][(size_t)l];
            // ---- dZ of this layer: (the loss's gradient + the next layer's data gradient) x LeakyReLU'
            if (l == nl - 1) {  // the output conv has no activation: dZ = dY
                for (int gi = 0; gi < L.groups; ++gi) {
                    float* dz = ws + bb.Y + (size_t)gi * bb.y_stride;
                    const float* dy = douts[obase[si][(size_t)l] + gi];
                    if (dy) HIP_TRY(hipMemcpyAsync(dz, dy, (size_t)tb.M * L.Np * sizeof(float), hipMemcpyDeviceToDevice, stream));
                    else HIP_TRY(hipMemsetAsync(dz, 0, (size_t)tb.M * L.Np * sizeof(float), stream));
                }
            } else {
                if (L.groups > 16) return fail(HIFICAR_E_INVALID, "discriminator: more than 16 groups in %s", L.base.c_str());
                const DiscLayer& N = s.layers[(size_t)l + 1];
                Col2imParams cp;
                memset(&cp, 0, sizeof(cp));
                cp.dA = ws + p.bwd[si][(size_t)l + 1].A;
                cp.da_gstride = (long long)p.bwd[si][(size_t)l + 1].a_stride;
                for (int gi = 0; gi < L.groups; ++gi) cp.dy[gi] = douts[obase[si][(size_t)l] + gi];
                cp.y = tape + tb.Y;
                cp.dz = ws + bb.Y;
                cp.y_gstride = (long long)tb.y_stride;
                cp.per_group = tb.M * L.Np;
                cp.total = cp.per_group * L.groups;
                cp.np = L.Np;
                cp.cout_g_prev = L.cout_g;
                cp.L_in = g.L[(size_t)l + 1];
                cp.L_out = g.L[(size_t)l + 2];
                cp.kt = N.k;
                cp.stride = N.stride;
                cp.pad = N.pad;
                cp.cin_g = N.cin_g;
                cp.Kg_pad = N.Kg_pad;
                cp.slope = s.slope;
                if (p.bwd[si][(size_t)l + 1].Lp) {  // dX [group][seq][Lp][cin_g] at padded positions
                    cp.win = 1;
                    cp.win_rows = p.bwd[si][(size_t)l + 1].Lp;
                    cp.win_pitch = N.cin_g;
                    cp.win_off = N.pad;
                }
                bool vec4 = d->col2im_vec4 && cp.np % 4 == 0 && cp.cout_g_prev % 4 == 0 && cp.cin_g % 4 == 0 && cp.Kg_pad % 4 == 0 && cp.y_gstride % 4 == 0 &&
                            cp.da_gstride % 4 == 0 && (!cp.win || cp.win_pitch % 4 == 0) && cp.per_group < (1LL << 31) &&
                            (reinterpret_cast<uintptr_t>(cp.dA) | reinterpret_cast<uintptr_t>(cp.y) | reinterpret_cast<uintptr_t>(cp.dz)) % 16 == 0;
                for (int gi = 0; gi < L.groups; ++gi) vec4 = vec4 && reinterpret_cast<uintptr_t>(cp.dy[gi]) % 16 == 0;
                ProfScope prof(h, stream, h->profile_detail ? "col2im_mask_kernel|" + L.base + (vec4 ? " v4" : " v1") : std::string("col2im_mask_kernel"), 0.0,
                               12.0 * cp.total);
                if (vec4) hipLaunchKernelGGL(col2im_mask4_kernel, dim3(ew_blocks(h, cp.per_group / 4), (unsigned)L.groups), dim3(256), 0, stream, cp);
                else hipLaunchKernelGGL(col2im_mask_kernel, dim3(ew_blocks(h, cp.total)), dim3(256), 0, stream, cp);
                HIP_TRY(hipGetLastError());
            }
            // ---- weight / bias gradients
            if (grads) {
                float* dW = grads + d->raw.offset(L.base + ".weight");
                float* dB = L.has_bias ? grads + d->raw.offset(L.base + ".bias") : nullptr;
                const DiscGroup& G = L.g[0];
                WgradJob job;
                job.L = &G.F;
                job.g = ws + bb.Y;
                job.gpitch = L.Np;
                job.a = tape + tb.A;
                job.apitch = L.Kg_pad;
                job.dW = dW;
                job.db = dB;
                job.gemm_cin = L.cin_g;
                job.gemm_kt = L.k;
                job.zg = L.groups;  // every group of a grouped conv in the same launches
                job.zs_g = (long long)bb.y_stride;
                job.zs_a = (long long)tb.a_stride;
                job.zs_dW = (long long)L.cout_g * L.cin_g * L.k;
                job.zs_db = L.cout_g;
                if (tb.Lp) {  // polyphase-input form: the all-taps kernel over the rows of X, dW' [tap q][co][r * cin_g + c] -> (co, c, stride q + r)
                    job.L = &G.P;
                    job.apitch = L.stride * L.cin_g;
                    job.a_seq_pitch = (long long)tb.Lp * L.cin_g;
                    job.a_rows = tb.Lp / L.stride;
                    job.gemm_cin = job.gemm_kt = 0;
                    job.poly_s = L.stride;
                    job.poly_cin = L.cin_g;
                    job.poly_k = L.k;
                }
                if ((rc = tb.Lp ? launch_wgrad_n(h, &job, 1, g.nseq, g.L[(size_t)l + 1], bw, stream) : launch_wgrad_n(h, &job, 1, 1, (int)tb.M, bw, stream)) !=
                    HIFICAR_OK)
                    return rc;
            }
            // ---- data gradient with respect to the im2col matrix (needed below layer 0 only when dx is wanted)
            if (bb.Lp) {  // dX4 rows = L_out + ntaps - 1 (more than the dZ rows they are computed from: x_rows)
                ConvIO io{};
                io.xs = reinterpret_cast<const char*>(ws + bb.Y);
                io.y = ws + bb.A;
                io.x_rows = g.L[(size_t)l + 1];
                io.x_seq_bytes = (long long)g.L[(size_t)l + 1] * L.Np * 4;
                ConvRep zr;
                zr.n = L.groups;
                zr.zs_x = (long long)bb.y_stride * 4;
                zr.zs_y = (long long)bb.a_stride;
                zr.zs_w = (long long)pack_w32_elems(L.g[0].Q, L.g[0].Q.chunk16) * 4;
                zr.zs_b = L.g[0].Q.cout_total;
                if ((rc = launch_conv1(h, L.g[0].Q, g.nseq, bb.Lp / L.stride, io, 0.f, rg, stream, zr)) != HIFICAR_OK) return rc;
            } else if (l > 0 || dx) {
                ConvIO io{};
                io.xs = reinterpret_cast<const char*>(ws + bb.Y);
                io.y = ws + bb.A;
                ConvRep zr;
                zr.n = L.groups;
                zr.zs_x = (long long)bb.y_stride * 4;
                zr.zs_y = (long long)bb.a_stride;
                zr.zs_w = (long long)pack_w32_elems(L.g[0].D, L.g[0].D.chunk16) * 4;
                zr.zs_b = L.g[0].D.cout_total;
                if ((rc = launch_conv1(h, L.g[0].D, 1, (int)tb.M, io, 0.f, rg, stream, zr)) != HIFICAR_OK) return rc;
            }
        }
        if ((rc = flush_reduce(h, pending, stream)) != HIFICAR_OK) return rc;  // every weight / bias gradient reduction of this sub-discriminator
        if (grads && d->raw.bucket_fn) d->raw.bucket_fn((int)si, stream, d->raw.bucket_user);  // this sub-discriminator's parameter gradients are enqueued
        if (!dx) continue;
        // ---- gradient of this sub-discriminator's input signal
        const DiscLayer& L0 = s.layers[0];
        SignalGradParams sp;
        memset(&sp, 0, sizeof(sp));
        sp.dA = ws + p.bwd[si][0].A;
        sp.T = g.T_sub;
        sp.period = s.period;
        sp.L_in = g.L[0];
        sp.L_out = g.L[1];
        sp.kt = L0.k;
        sp.stride = L0.stride;
        sp.pad = L0.pad;
        sp.Kg_pad = L0.Kg_pad;
        sp.total = (long long)B * g.T_sub;
        sp.dx = ws + p.dsig[si];
        sp.accumulate = 0;
        ProfScope prof(h, stream, "signal_grad_kernel", 0.0, 8.0 * sp.total);
        hipLaunchKernelGGL(signal_grad_kernel, dim3(ew_blocks(h, sp.total)), dim3(256), 0, stream, sp);
        HIP_TRY(hipGetLastError());
    }
    return HIFICAR_OK;
    }();
    {
        const int rcj = disc_join(d, main_stream);
        if (rc != HIFICAR_OK) return rc;
        if (rcj != HIFICAR_OK) return rcj;
    }
    stream = main_stream;
    if (dx) {
        // dx = the sub-discriminators' signal gradients summed in a fixed order; the scale discriminators' flow back through the
        // AvgPool1d chain: scale s -> scale s - 1 -> ... -> the input
        std::vector<int> Ts((size_t)std::max(n_scales, 1), T);
        for (int i = 1; i < n_scales; ++i) Ts[(size_t)i] = disc_out_len(Ts[(size_t)i - 1], d->cfg.pool_kernel, d->cfg.pool_stride, d->cfg.pool_pad);
        std::vector<const float*> dscale((size_t)std::max(n_scales, 1), nullptr);
        SumParams sm;
        memset(&sm, 0, sizeof(sm));
        for (size_t si = 0; si < d->subs.size(); ++si) {
            const DiscSub& s = d->subs[si];
            if (s.period == 0 && s.scale > 0) dscale[(size_t)s.scale] = ws + p.dsig[si];
            else sm.src[sm.n++] = ws + p.dsig[si];
        }
        sm.dst = dx;
        sm.total = (long long)B * T;
        {
            ProfScope prof(h, stream, "sum_kernel", 0.0, 4.0 * sm.total * (sm.n + 1));
            hipLaunchKernelGGL(sum_kernel, dim3(ew_blocks(h, sm.total)), dim3(256), 0, stream, sm);
            HIP_TRY(hipGetLastError());
        }
        for (int i = n_scales - 1; i >= 1; --i) {
            if (!dscale[(size_t)i]) continue;
            PoolParams pp;
            pp.src = dscale[(size_t)i];
            pp.dst = i == 1 ? dx : const_cast<float*>(dscale[(size_t)i - 1]);
            pp.L_src = Ts[(size_t)i];
            pp.L_dst = Ts[(size_t)i - 1];
            pp.total = (long long)B * pp.L_dst;
            pp.kernel = d->cfg.pool_kernel;
            pp.stride = d->cfg.pool_stride;
            pp.pad = d->cfg.pool_pad;
            pp.accumulate = 1;
            ProfScope prof(h, stream, "avgpool_bwd_kernel", 0.0, 12.0 * pp.total);
            hipLaunchKernelGGL(avgpool_bwd_kernel, dim3(ew_blocks(h, pp.total)), dim3(256), 0, stream, pp);
            HIP_TRY(hipGetLastError());
        }
    }
    // Mark the end of this call on its stream: a following call on ANOTHER stream waits for this point only (enter_stream), not for what
    // the caller has enqueued on this stream since — the generator's own backward, when the next call is the early real pass of the
    // discriminator update on a side stream (articulatory_amd/models/discriminator.py::start_real_gradient).
    if (!h->done_ev) HIP_TRY(hipEventCreateWithFlags(&h->done_ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(h->done_ev, main_stream));
    h->done_valid = true;
    h->done_stream = main_stream;
    return HIFICAR_OK;
}

// ------------------------------------------------------------------------------------------------
// GAN losses on the forward tapes (loss_kernel): values and the gradient buffers hificar_disc_backward_flat consumes.
// ------------------------------------------------------------------------------------------------
struct DoutLayout {
    std::vector<size_t> off;  // [output buffer] floats
    size_t partials = 0;
    size_t total = 0;
};

static DoutLayout dout_layout(const hificar_disc* d, const DiscPlan& p) {
    DoutLayout L;
    size_t off = 0;
    for (size_t si = 0; si < d->subs.size(); ++si)
        for (size_t l = 0; l < d->subs[si].layers.size(); ++l)
            for (int g = 0; g < d->subs[si].layers[l].groups; ++g) {
                L.off.push_back(off);
                off += round_up_sz((size_t)p.tape[si][l].M * d->subs[si].layers[l].Np, 256);
            }
    L.partials = off;
    off += L.off.size() * kLossChunks * 2;
    L.total = off;
    return L;
}

extern "C" size_t hificar_disc_dout_floats(const hificar_disc* d, int B, int T) {
    if (!d || B < 1 || T < 2) return 0;
    return dout_layout(d, disc_plan(d, B, T)).total;
}

// mode 0: generator side — adversarial loss of the FAKE pass's final outputs + feature matching against `tape_ref` (the REAL pass;
//         NULL: no feature matching): values = {adv, fm, lambda_adv * (adv + lambda_feat_match * fm)} (train.py:341-362)
// mode 1: discriminator side, FAKE pass: values = {fake loss, 0, fake loss};  mode 2: REAL pass: values = {real loss, 0, real loss}
// douts (hificar_disc_dout_floats floats): d(values[2]) / d(every output buffer of `tape`), for hificar_disc_backward_flat.
extern "C" int hificar_disc_loss(hificar_disc* d, const hificar_gan_loss_config* cfg, int mode, const void* tape_, const void* tape_ref_, int B, int T,
                                 float* values3, float* douts, void* stream_) {
    if (!d || !cfg || !tape_ || !values3 || !douts || mode < 0 || mode > 2) return fail(HIFICAR_E_INVALID, "hificar_disc_loss: bad argument");
    hificar_engine* h = &d->eng;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    int rc;
    if ((rc = enter_stream(h, stream)) != HIFICAR_OK) return rc;
    const bool fm = mode == 0 && tape_ref_ != nullptr;
    char key[160];
    snprintf(key, sizeof(key), "%d|%d|%d|%d|%d|%d|%d|%d|%d|%.9g|%.9g", B, T, mode, fm ? 1 : 0, cfg->loss_type, cfg->average_by_discriminators,
             cfg->fm_average_by_layers, cfg->fm_average_by_discriminators, cfg->fm_include_final_outputs, cfg->lambda_adv, cfg->lambda_feat_match);
    auto it = d->loss_tables.find(key);
    if (it == d->loss_tables.end()) {
        const DiscPlan p = disc_plan(d, B, T);
        const DoutLayout dl = dout_layout(d, p);
        std::vector<LossEntry> entries;
        hificar_disc::LossTable tab;
        const double n_disc = (double)d->subs.size();
        const double lam_adv = mode == 0 ? cfg->lambda_adv : 1.0, lam_fm = cfg->lambda_feat_match;
        int oi = 0;
        for (size_t si = 0; si < d->subs.size(); ++si) {
            const int nl = (int)d->subs[si].layers.size();
            const int n_fm_layers = nl - (cfg->fm_include_final_outputs ? 0 : 1);
            for (int l = 0; l < nl; ++l) {
                const DiscLayer& L = d->subs[si].layers[(size_t)l];
                const double numel = (double)p.tape[si][(size_t)l].M * L.cout;  // all groups
                for (int g = 0; g < L.groups; ++g, ++oi) {
                    LossEntry e;
                    memset(&e, 0, sizeof(e));
                    e.y_off = (long long)(p.tape[si][(size_t)l].Y + (size_t)g * p.tape[si][(size_t)l].y_stride);
                    e.d_off = (long long)dl.off[(size_t)oi];
                    e.total = p.tape[si][(size_t)l].M * L.Np;
                    e.pitch = L.Np;
                    e.channels = L.cout_g;
                    if (l == nl - 1) {
                        const bool mse = cfg->loss_type == 0;
                        e.adv_kind = mode == 0 ? (mse ? 1 : 3) : mode == 1 ? (mse ? 2 : 5) : (mse ? 1 : 4);
                        e.c_adv = (float)((cfg->average_by_discriminators ? 1.0 / n_disc : 1.0) / numel);
                        e.w_adv = (float)(lam_adv * (cfg->average_by_discriminators ? 1.0 / n_disc : 1.0) / numel);
                    }
                    if (fm && l < n_fm_layers) {
                        const double c = (cfg->fm_average_by_layers ? 1.0 / n_fm_layers : 1.0) * (cfg->fm_average_by_discriminators ? 1.0 / n_disc : 1.0) / numel;
                        e.c_fm = (float)c;
                        e.w_fm = (float)(lam_adv * lam_fm * c);
                    }
                    if (e.adv_kind == 0 && e.c_fm == 0.f) continue;  // (not w_fm: with lambda 0 the buffer still gets its zero gradient)
                    entries.push_back(e);
                    tab.out_index.push_back(oi);
                }
            }
        }
        tab.n = (int)entries.size();
        if ((rc = device_table(h, entries, &tab.d_entries)) != HIFICAR_OK) return rc;
        if (d->loss_tables.size() > 64) d->loss_tables.clear();  // (device tables stay allocated until the handle goes: tiny)
        it = d->loss_tables.emplace(key, tab).first;
    }
    const hificar_disc::LossTable& tab = it->second;
    const DoutLayout dl = dout_layout(d, disc_plan(d, B, T));
    {
        ProfScope prof(h, stream, "loss_kernel", 0.0, 0.0);
        hipLaunchKernelGGL(loss_kernel, dim3(kLossChunks, tab.n), dim3(256), 0, stream, tab.d_entries, static_cast<const float*>(tape_),
                           fm ? static_cast<const float*>(tape_ref_) : nullptr, douts, douts + dl.partials);
    }
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(256), 0, stream, tab.d_entries, tab.n, douts + dl.partials, values3,
                       mode == 0 ? cfg->lambda_adv : 1.f, mode == 0 ? cfg->lambda_feat_match : 0.f);
    HIP_TRY(hipGetLastError());
    return HIFICAR_OK;
}

// hificar_disc_backward on the gradient buffer of hificar_disc_loss (`mode` / `with_fm` as in that call: they say which output buffers
// carry a gradient).
extern "C" int hificar_disc_backward_flat(hificar_disc* d, const float* douts, int mode, int with_fm, int fm_include_final_outputs, int B, int T,
                                          const void* tape, size_t tape_bytes, float* grads, float* dx, void* ws, size_t ws_bytes, void* stream) {
    if (!d || !douts) return fail(HIFICAR_E_INVALID, "hificar_disc_backward_flat: null argument");
    const DiscPlan p = disc_plan(d, B, T);
    const DoutLayout dl = dout_layout(d, p);
    std::vector<const float*> ptrs(dl.off.size(), nullptr);
    int oi = 0;
    for (size_t si = 0; si < d->subs.size(); ++si) {
        const int nl = (int)d->subs[si].layers.size();
        for (int l = 0; l < nl; ++l)
            for (int g = 0; g < d->subs[si].layers[(size_t)l].groups; ++g, ++oi) {
                const bool fm = mode == 0 && with_fm && l < nl - (fm_include_final_outputs ? 0 : 1);
                if (l == nl - 1 || fm) ptrs[(size_t)oi] = douts + dl.off[(size_t)oi];
            }
    }
    return hificar_disc_backward(d, ptrs.data(), B, T, tape, tape_bytes, grads, dx, ws, ws_bytes, stream);
}
