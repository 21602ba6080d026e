// The HuBERT encoder, "large" family (the `transformers` library's HubertModel with feat_extract_norm = "layer", do_stable_layer_norm = True):
// waveforms (B, L) at 16 kHz -> hidden states (B, hidden, Tmax) at 50 Hz, eval mode.
//   statistics   per utterance mean and 1 / sqrt(var + eps) of its samples                         hubert_stats_kernel, hubert_frames_kernel
//   layer 0      Conv1d(1 -> C, k 10, s 5) + LayerNorm + GELU, the normalisation folded into its reads   hubert_conv0_kernel
//   layers 1-6   Conv1d(C -> C, k 3 | 2, s 2): the channels-last rows [P][C] read as [P / 2][2 C], a stride-1 conv of ceil(k / 2) taps whose
//                weights were re-laid at hand-over (missing slots zero; the engine's polyphase-input form, ConvParams::x_rows)      conv engine
//                + LayerNorm + GELU per row                                                       hubert_ln_kernel<true>
//   projection   LayerNorm (the config's eps) + Linear(C, H)                                      hubert_ln_kernel, conv engine
//   positional   grouped 128-tap conv + bias + GELU, added to the stream                          hubert_posconv_kernel
//   per layer    LN, q | k | v as ONE GEMM (N = 3 H), attention, W_o + residual                   hubert_ln_kernel, conv engine, hubert_attn_kernel
//                LN, W_1, GELU (a pass of its own), W_2 + residual                                hubert_ln_kernel, conv engine, hubert_gelu_kernel
//   output       the encoder's LayerNorm (layer = -1), rows -> (B, H, Tmax) with zeros past a length     hubert_ln_kernel, xfmr_out_kernel
// The extractor needs no ragged context: a frame inside an utterance reads samples inside it only, and the rows past its frames — finite
// garbage formed from the zero padding — are never read by a valid row (a zero-weight slot reads at most the finite slack row).  It runs over
// sub-batches of utterances, so the workspace never holds a whole batch's layer-0 rows.  Everything behind it runs under the ragged context
// (frames per utterance): rows at or past a sequence's frames read as zeros in the GEMMs and are never written.  Exact fp32, split-K off.
//
// bf16x3 (hificar_hubert_set_precision, inference only): every GEMM on the conv engine — extractor layers 1 - 6, the projection, q | k | v,
// out_proj, intermediate_dense, output_dense — runs in the engine's bf16x3 kernels, whose input is "split rows" [hi: C bf16 | lo: C bf16]
// (4 C bytes per row, as fp32 rows) written by whatever produces it; there is no split pass of its own:
//   hubert_conv0_kernel<true>          split WINDOW rows [hi: 2 C | lo: 2 C] of two positions, layer 1's operand, in ws.ea
//   hubert_ln_kernel<true, true>       behind layers 1 - 5: conv i reads ws.ea and writes fp32 rows to ws.eb; the LayerNorm + GELU reads ws.eb and
//                                      writes layer i + 1's split window rows back into ws.ea (P[i] <= P[i - 1]: it fits; a position's bytes
//                                      interleave with its neighbour's, so the pass cannot be in place).  Behind layer 6: fp32, as ever
//   hubert_ln_kernel<false, true>      the projection's LayerNorm (in place over ws.feat) and the two per layer: split rows only — no later
//                                      kernel reads those rows as fp32
//   hubert_attn_kernel<64, true>       split rows for out_proj
//   hubert_gelu_split_kernel           split rows of GELU(W_1 n + b), in place over the wide buffer: one workgroup holds a row
// The waveform statistics, layer 0, every LayerNorm and GELU, the positional conv, the attention, biases, residual adds and the residual
// stream stay fp32.  No buffer grows: a split row takes its fp32 row's bytes.  The tap "extractor.0" exists as split rows only.
//
// bf16x3a (HIFICAR_PREC_BF16X3A): bf16x3 with the attention's two products on bf16 MFMAs too (hificar_hubert_attn16.hip.h).  The q | k | v
// GEMM writes split rows only ([hi: 3 H bf16 | lo: 3 H bf16], the bytes of the fp32 row).  The conv engine sees a bf16x3 handle.
//
// WavLM (hificar_hubert_set_rel_bias; f32 and bf16x3): each layer's first LayerNorm also forms the attention's gates from the row it holds
// (hubert_ln_kernel<false, SPLIT, true>, into ws.gates: (B, heads, T), one layer's, reused), and the attention adds
// gate[b, h, q] bias_d[h][clamp(k - q)] to its scores (hubert_attn_kernel<64, SPLIT, true>); bias_d is folded at finalize from layer 0's
// rel_attn_embed and the caller's bucket map.  Without the call nothing here differs from the above.

constexpr int kHubExtLayers = 7;
static const int kHubExtK[kHubExtLayers] = {10, 3, 3, 3, 3, 2, 2};
constexpr size_t kHubExtBudget = (size_t)512 << 20;  // bytes of layer-0 rows per extractor sub-batch

struct HubertEncLayer {
    ConvLayer qkv, wo, l1, l2;
    float* d_ln[4] = {nullptr, nullptr, nullptr, nullptr};  // layer_norm.weight, .bias, final_layer_norm.weight, .bias
    float* d_gate[3] = {nullptr, nullptr, nullptr};         // rel_bias: gru_rel_pos_linear.weight (8, 64), .bias (8), gru_rel_pos_const (heads)
};

struct hificar_hubert {
    hificar_hubert_config cfg;
    hificar_engine eng;
    WeightIntake weights;
    ConvLayer ext[kHubExtLayers];  // [1 .. 6]: the strided convs in window form ([0] unused: layer 0 has its own kernel)
    ConvLayer proj;
    std::vector<HubertEncLayer> enc;  // sized once, in hificar_hubert_create (launch plans are keyed by the layers' addresses)
    float* d_w0 = nullptr;            // layer 0's weight [10][C] and bias [C]
    float* d_b0 = nullptr;
    float* d_ext_ln[kHubExtLayers][2] = {};
    float* d_fp_ln[2] = {nullptr, nullptr};
    float* d_enc_ln[2] = {nullptr, nullptr};
    float* d_pos_w = nullptr;  // hubert_posconv_kernel's lane-ordered weights
    float* d_pos_b = nullptr;
    // hificar_hubert_set_rel_bias (WavLM): the attention adds gate[b, h, q] bias_d[h][clamp(k - q)] to its scores
    bool rel_bias = false;
    int num_buckets = 0, max_distance = 0;
    std::vector<int32_t> bucket_of;  // [2 max_distance + 1], host
    float* d_bias = nullptr;         // [heads][2 max_distance + 1]: rel_attn_embed folded with bucket_of at finalize
    int precision = HIFICAR_PREC_F32;  // hificar_hubert_set_precision: which fragments finalize packs and which kernels the forward launches
    bool finalized = false;
    int sub_batch = 0;  // hificar_hubert_debug_sub_batch: utterances per extractor sub-batch (0: by kHubExtBudget)
    TapTable taps;
};

// positions per sequence behind every extractor layer for L samples (T), and the rows its buffer holds (P: T rounded up to whole windows of two)
struct HubertDims {
    int T[kHubExtLayers], P[kHubExtLayers];
};
static bool hubert_dims(int L, HubertDims* d) {
    if (L < HIFICAR_HUBERT_MIN_SAMPLES) return false;
    d->T[0] = (L - 10) / 5 + 1;
    for (int i = 1; i < kHubExtLayers; ++i) d->T[i] = (d->T[i - 1] - kHubExtK[i]) / 2 + 1;
    for (int i = 0; i < kHubExtLayers; ++i) d->P[i] = i + 1 < kHubExtLayers ? round_up(d->T[i], 2) : d->T[i];
    return true;
}

static const char* const kHubRelBiasA16 =
    "HuBERT: the gated relative position bias (WavLM) is not built for bf16x3a: hubert_attn16_kernel has no bias term (f32 and bf16x3 are built)";

// the handle's GEMMs run in the engine's bf16x3 kernels (bf16x3 and bf16x3a differ in the attention alone)
static bool hubert_x3(const hificar_hubert* g) { return g->precision != HIFICAR_PREC_F32; }

static bool hubert_pos_group_built(int G) { return G == 8 || G == 16 || G == 32 || G == 48 || G == 64; }

template <class Fn>
static hipError_t hubert_by_group(int G, Fn&& fn) {
    switch (G) {
        case 8: return fn(std::integral_constant<int, 8>());
        case 16: return fn(std::integral_constant<int, 16>());
        case 32: return fn(std::integral_constant<int, 32>());
        case 48: return fn(std::integral_constant<int, 48>());
        case 64: return fn(std::integral_constant<int, 64>());
    }
    return hipErrorInvalidValue;
}

static int hubert_plan(ConvLayer& L, const std::string& name, int cin, int cout, int K) {
    L.name = name;
    L.cin = cin;
    L.cin_pad = cin;
    L.cout = cout;
    L.K = K;
    L.padding = 0;  // (a window conv's tap j reads row t + j)
    return plan_layer(L);
}

extern "C" int hificar_hubert_create(const hificar_hubert_config* cfg, hificar_hubert** out) {
    if (!cfg || !out) return fail(HIFICAR_E_INVALID, "hificar_hubert_create: null argument");
    const hificar_hubert_config& c = *cfg;
    if (c.conv_dim < 32 || c.conv_dim > HIFICAR_HUBERT_MAX_CONV || c.conv_dim % 32 != 0)
        return fail(HIFICAR_E_INVALID, "HuBERT: conv_dim=%d unsupported (multiples of 32 up to %d)", c.conv_dim, HIFICAR_HUBERT_MAX_CONV);
    if (c.hidden_size < 1 || c.hidden_size % kHubPosGroups != 0 || !hubert_pos_group_built(c.hidden_size / kHubPosGroups))
        return fail(HIFICAR_E_INVALID, "HuBERT: hidden_size=%d unsupported (128, 256, 512, 768 or 1024: 16 positional groups of 8 .. 64 channels)", c.hidden_size);
    if (c.num_attention_heads * HIFICAR_HUBERT_HEAD_DIM != c.hidden_size)
        return fail(HIFICAR_E_INVALID, "HuBERT: %d heads of hidden_size=%d: the attention kernel is built for head size %d only", c.num_attention_heads,
                    c.hidden_size, HIFICAR_HUBERT_HEAD_DIM);
    if (c.intermediate_size < 32 || c.intermediate_size > HIFICAR_HUBERT_MAX_FFN || c.intermediate_size % 32 != 0)
        return fail(HIFICAR_E_INVALID, "HuBERT: intermediate_size=%d unsupported (multiples of 32 up to %d)", c.intermediate_size, HIFICAR_HUBERT_MAX_FFN);
    if (c.num_hidden_layers < 1 || c.num_hidden_layers > HIFICAR_HUBERT_MAX_LAYERS)
        return fail(HIFICAR_E_INVALID, "HuBERT: num_hidden_layers=%d out of range (1 .. %d)", c.num_hidden_layers, HIFICAR_HUBERT_MAX_LAYERS);
    if (!(c.layer_norm_eps > 0.f) || !(c.norm_eps >= 0.f)) return fail(HIFICAR_E_INVALID, "HuBERT: layer_norm_eps must be positive and norm_eps not negative");
    hificar_hubert* g = new hificar_hubert();
    g->cfg = c;
    const int64_t C = c.conv_dim, H = c.hidden_size, I = c.intermediate_size;
    for (int i = 0; i < kHubExtLayers; ++i) {
        const std::string b = "feature_extractor.conv_layers." + std::to_string(i) + ".";
        g->weights.expected[b + "conv.weight"] = {C, i == 0 ? 1 : C, kHubExtK[i]};
        if (c.conv_bias) g->weights.expected[b + "conv.bias"] = {C};
        g->weights.expected[b + "layer_norm.weight"] = {C};
        g->weights.expected[b + "layer_norm.bias"] = {C};
    }
    g->weights.expected["feature_projection.layer_norm.weight"] = {C};
    g->weights.expected["feature_projection.layer_norm.bias"] = {C};
    g->weights.expected["feature_projection.projection.weight"] = {H, C};
    g->weights.expected["feature_projection.projection.bias"] = {H};
    g->weights.expected["encoder.pos_conv_embed.conv.weight_g"] = {1, 1, kHubPosTaps};
    g->weights.expected["encoder.pos_conv_embed.conv.weight_v"] = {H, H / kHubPosGroups, kHubPosTaps};
    g->weights.expected["encoder.pos_conv_embed.conv.bias"] = {H};
    g->weights.expected["encoder.layer_norm.weight"] = {H};
    g->weights.expected["encoder.layer_norm.bias"] = {H};
    for (int l = 0; l < c.num_hidden_layers; ++l) {
        const std::string b = "encoder.layers." + std::to_string(l) + ".";
        for (const char* w : {"q_proj", "k_proj", "v_proj", "out_proj"}) {
            g->weights.expected[b + "attention." + w + ".weight"] = {H, H};
            g->weights.expected[b + "attention." + w + ".bias"] = {H};
        }
        for (const char* n : {"layer_norm", "final_layer_norm"})
            for (const char* t : {".weight", ".bias"}) g->weights.expected[b + n + t] = {H};
        g->weights.expected[b + "feed_forward.intermediate_dense.weight"] = {I, H};
        g->weights.expected[b + "feed_forward.intermediate_dense.bias"] = {I};
        g->weights.expected[b + "feed_forward.output_dense.weight"] = {H, I};
        g->weights.expected[b + "feed_forward.output_dense.bias"] = {H};
    }
    g->enc.resize((size_t)c.num_hidden_layers);
    int rc = HIFICAR_OK;
    for (int i = 1; i < kHubExtLayers && rc == HIFICAR_OK; ++i)
        rc = hubert_plan(g->ext[i], "feature_extractor.conv_layers." + std::to_string(i) + ".conv#window", 2 * c.conv_dim, c.conv_dim, (kHubExtK[i] + 1) / 2);
    if (rc == HIFICAR_OK) rc = hubert_plan(g->proj, "feature_projection.projection", c.conv_dim, c.hidden_size, 1);
    for (int l = 0; l < c.num_hidden_layers && rc == HIFICAR_OK; ++l) {
        const std::string b = "encoder.layers." + std::to_string(l);
        HubertEncLayer& E = g->enc[(size_t)l];
        rc = hubert_plan(E.qkv, b + ".attention#qkv", c.hidden_size, 3 * c.hidden_size, 1);
        if (rc == HIFICAR_OK) rc = hubert_plan(E.wo, b + ".attention.out_proj", c.hidden_size, c.hidden_size, 1);
        if (rc == HIFICAR_OK) rc = hubert_plan(E.l1, b + ".feed_forward.intermediate_dense", c.hidden_size, c.intermediate_size, 1);
        if (rc == HIFICAR_OK) rc = hubert_plan(E.l2, b + ".feed_forward.output_dense", c.intermediate_size, c.hidden_size, 1);
    }
    if (rc != HIFICAR_OK) {
        delete g;
        return rc;
    }
    *out = g;
    return HIFICAR_OK;
}

extern "C" void hificar_hubert_destroy(hificar_hubert* g) {
    if (!g) return;
    engine_close(&g->eng);
    delete g;
}

extern "C" hificar_engine* hificar_hubert_engine(hificar_hubert* g) { return g ? &g->eng : nullptr; }

extern "C" int hificar_hubert_frames(const hificar_hubert* g, int L) {
    (void)g;
    return L >= HIFICAR_HUBERT_MIN_SAMPLES ? (L - 400) / 320 + 1 : 0;
}

extern "C" int hificar_hubert_set_weight(hificar_hubert* g, const char* name, const float* data, const int64_t* shape, int ndim) {
    if (!g || !name || !data || !shape) return fail(HIFICAR_E_INVALID, "hificar_hubert_set_weight: null argument");
    if (g->finalized) return fail(HIFICAR_E_STATE, "hificar_hubert_set_weight(%s) after hificar_hubert_finalize", name);
    return g->weights.set(name, data, shape, ndim);
}

extern "C" int hificar_hubert_set_precision(hificar_hubert* g, int precision) {
    if (!g) return fail(HIFICAR_E_INVALID, "hificar_hubert_set_precision: null handle");
    if (precision != HIFICAR_PREC_F32 && precision != HIFICAR_PREC_BF16X3 && precision != HIFICAR_PREC_BF16X3A)
        return fail(HIFICAR_E_INVALID, "unknown precision %d", precision);
    if (g->finalized)
        return fail(HIFICAR_E_STATE, "hificar_hubert_set_precision after hificar_hubert_finalize: the weights are packed for %s only; make a new handle",
                    xfmr_precision_name(g->precision));
    if (precision == HIFICAR_PREC_BF16X3A && g->rel_bias) return fail(HIFICAR_E_INVALID, "%s", kHubRelBiasA16);
    g->precision = precision;
    return HIFICAR_OK;
}

extern "C" int hificar_hubert_set_rel_bias(hificar_hubert* g, int num_buckets, int max_distance, const int32_t* bucket_of_distance) {
    if (!g || !bucket_of_distance) return fail(HIFICAR_E_INVALID, "hificar_hubert_set_rel_bias: null argument");
    if (g->finalized) return fail(HIFICAR_E_STATE, "hificar_hubert_set_rel_bias after hificar_hubert_finalize");
    if (num_buckets < 2 || num_buckets % 2 != 0 || num_buckets > HIFICAR_HUBERT_MAX_BUCKETS)
        return fail(HIFICAR_E_INVALID, "hificar_hubert_set_rel_bias: num_buckets=%d must be even and in 2 .. %d", num_buckets, HIFICAR_HUBERT_MAX_BUCKETS);
    if (max_distance < 1 || max_distance > HIFICAR_HUBERT_MAX_DISTANCE)
        return fail(HIFICAR_E_INVALID, "hificar_hubert_set_rel_bias: max_distance=%d outside 1 .. %d", max_distance, HIFICAR_HUBERT_MAX_DISTANCE);
    if (g->precision == HIFICAR_PREC_BF16X3A) return fail(HIFICAR_E_INVALID, "%s", kHubRelBiasA16);
    for (int i = 0; i < 2 * max_distance + 1; ++i)
        if (bucket_of_distance[i] < 0 || bucket_of_distance[i] >= num_buckets)
            return fail(HIFICAR_E_INVALID, "hificar_hubert_set_rel_bias: bucket_of_distance[%d]=%d outside 0 .. %d", i, (int)bucket_of_distance[i], num_buckets - 1);
    if (g->rel_bias) g->weights.expected.erase("encoder.layers.0.attention.rel_attn_embed.weight");  // (a second call: the table's shape may differ)
    g->weights.tensors.erase("encoder.layers.0.attention.rel_attn_embed.weight");
    g->rel_bias = true;
    g->num_buckets = num_buckets;
    g->max_distance = max_distance;
    g->bucket_of.assign(bucket_of_distance, bucket_of_distance + 2 * max_distance + 1);
    const int64_t heads = g->cfg.num_attention_heads;
    g->weights.expected["encoder.layers.0.attention.rel_attn_embed.weight"] = {num_buckets, heads};
    for (int l = 0; l < g->cfg.num_hidden_layers; ++l) {
        const std::string b = "encoder.layers." + std::to_string(l) + ".attention.";
        g->weights.expected[b + "gru_rel_pos_linear.weight"] = {8, kHubHeadDim};
        g->weights.expected[b + "gru_rel_pos_linear.bias"] = {8};
        g->weights.expected[b + "gru_rel_pos_const"] = {1, heads, 1, 1};
    }
    return HIFICAR_OK;
}

extern "C" int hificar_hubert_finalize(hificar_hubert* g) {
    if (!g) return fail(HIFICAR_E_INVALID, "hificar_hubert_finalize: null handle");
    if (g->finalized) return HIFICAR_OK;
    if (const int missing = g->weights.check_complete()) return missing;
    hificar_engine* h = &g->eng;
    const int C = g->cfg.conv_dim, H = g->cfg.hidden_size, G = H / kHubPosGroups;
    int rc;
    const bool x3 = hubert_x3(g);
    h->precision = x3 ? HIFICAR_PREC_BF16X3 : HIFICAR_PREC_F32;  // (xfmr_pack goes by it)
    auto vec = [&](const std::string& name) -> const std::vector<float>& { return g->weights.data(name); };
    const std::vector<float> zeros_c((size_t)C, 0.f);
    for (int i = 0; i < kHubExtLayers; ++i) {
        const std::string b = "feature_extractor.conv_layers." + std::to_string(i) + ".";
        const std::vector<float>& W = vec(b + "conv.weight");
        const std::vector<float>* bias = g->cfg.conv_bias ? &vec(b + "conv.bias") : nullptr;
        if ((rc = upload(h, vec(b + "layer_norm.weight"), &g->d_ext_ln[i][0])) != HIFICAR_OK) return rc;
        if ((rc = upload(h, vec(b + "layer_norm.bias"), &g->d_ext_ln[i][1])) != HIFICAR_OK) return rc;
        if (i == 0) {  // [C][1][10] -> [10][C]
            std::vector<float> w0((size_t)kHubK0 * C);
            for (int o = 0; o < C; ++o)
                for (int k = 0; k < kHubK0; ++k) w0[(size_t)k * C + o] = W[(size_t)o * kHubK0 + k];
            if ((rc = upload(h, w0, &g->d_w0)) != HIFICAR_OK) return rc;
            if ((rc = upload(h, bias ? *bias : zeros_c, &g->d_b0)) != HIFICAR_OK) return rc;
            continue;
        }
        // window form: W'[o][slot C + c][tap] = W[o][c][2 tap + slot], zero where 2 tap + slot >= k
        const int k = kHubExtK[i], nt = (k + 1) / 2;
        HostTensor Ww;
        Ww.shape = {C, 2 * C, nt};
        Ww.data.assign((size_t)C * 2 * C * nt, 0.f);
        for (int o = 0; o < C; ++o)
            for (int c = 0; c < C; ++c)
                for (int j = 0; j < k; ++j) Ww.data[((size_t)o * 2 * C + (size_t)(j & 1) * C + c) * nt + (j >> 1)] = W[((size_t)o * C + c) * k + j];
        if ((rc = xfmr_pack(h, g->ext[i], Ww, bias)) != HIFICAR_OK) return rc;
    }
    if ((rc = upload(h, vec("feature_projection.layer_norm.weight"), &g->d_fp_ln[0])) != HIFICAR_OK) return rc;
    if ((rc = upload(h, vec("feature_projection.layer_norm.bias"), &g->d_fp_ln[1])) != HIFICAR_OK) return rc;
    if ((rc = pack_linear(h, g->proj, g->weights, "feature_projection.projection")) != HIFICAR_OK) return rc;
    if ((rc = upload(h, vec("encoder.layer_norm.weight"), &g->d_enc_ln[0])) != HIFICAR_OK) return rc;
    if ((rc = upload(h, vec("encoder.layer_norm.bias"), &g->d_enc_ln[1])) != HIFICAR_OK) return rc;
    {   // weight norm over dim 2 (w[:, :, k] = g[k] v[:, :, k] / ||v[:, :, k]||), folded in double, in the kernel's lane order:
        // [group][tap][NOB][G / 4][lane = 16 (cin & 3) + (cout & 15)], output channels past G zeros
        const std::vector<float>&gw = vec("encoder.pos_conv_embed.conv.weight_g"), &v = vec("encoder.pos_conv_embed.conv.weight_v");
        std::vector<double> scale(kHubPosTaps);
        for (int k = 0; k < kHubPosTaps; ++k) {
            double ss = 0.0;
            for (size_t e = 0; e < (size_t)H * G; ++e) ss += (double)v[e * kHubPosTaps + k] * (double)v[e * kHubPosTaps + k];
            scale[k] = (double)gw[k] / std::sqrt(ss);
        }
        const int NOB = (G + 15) / 16, NS = G / 4;
        std::vector<float> wp((size_t)kHubPosGroups * kHubPosTaps * NOB * NS * 64, 0.f);
        for (int grp = 0; grp < kHubPosGroups; ++grp)
            for (int k = 0; k < kHubPosTaps; ++k)
                for (int o = 0; o < G; ++o)
                    for (int c = 0; c < G; ++c) {
                        const size_t at = ((((size_t)grp * kHubPosTaps + k) * NOB + o / 16) * NS + c / 4) * 64 + (size_t)(c & 3) * 16 + (o & 15);
                        wp[at] = (float)((double)v[(((size_t)grp * G + o) * G + c) * kHubPosTaps + k] * scale[k]);
                    }
        if ((rc = upload(h, wp, &g->d_pos_w)) != HIFICAR_OK) return rc;
        if ((rc = upload(h, vec("encoder.pos_conv_embed.conv.bias"), &g->d_pos_b)) != HIFICAR_OK) return rc;
    }
    for (int l = 0; l < g->cfg.num_hidden_layers; ++l) {
        const std::string b = "encoder.layers." + std::to_string(l) + ".";
        HubertEncLayer& E = g->enc[(size_t)l];
        {   // q | k | v as one GEMM: the three weights and biases stacked
            HostTensor W;
            W.shape = {3 * H, H, 1};
            std::vector<float> bias;
            for (const char* w : {"q_proj", "k_proj", "v_proj"}) {
                const std::vector<float>&ws = vec(b + "attention." + w + ".weight"), &bs = vec(b + "attention." + w + ".bias");
                W.data.insert(W.data.end(), ws.begin(), ws.end());
                bias.insert(bias.end(), bs.begin(), bs.end());
            }
            if ((rc = xfmr_pack(h, E.qkv, W, &bias)) != HIFICAR_OK) return rc;
        }
        if ((rc = pack_linear(h, E.wo, g->weights, b + "attention.out_proj")) != HIFICAR_OK) return rc;
        if ((rc = pack_linear(h, E.l1, g->weights, b + "feed_forward.intermediate_dense")) != HIFICAR_OK) return rc;
        if ((rc = pack_linear(h, E.l2, g->weights, b + "feed_forward.output_dense")) != HIFICAR_OK) return rc;
        int i = 0;
        for (const char* n : {"layer_norm.weight", "layer_norm.bias", "final_layer_norm.weight", "final_layer_norm.bias"})
            if ((rc = upload(h, vec(b + n), &E.d_ln[i++])) != HIFICAR_OK) return rc;
        if (g->rel_bias) {
            i = 0;
            for (const char* n : {"attention.gru_rel_pos_linear.weight", "attention.gru_rel_pos_linear.bias", "attention.gru_rel_pos_const"})
                if ((rc = upload(h, vec(b + n), &E.d_gate[i++])) != HIFICAR_OK) return rc;
        }
    }
    if (g->rel_bias) {  // bias_d[h][d + D] = rel_attn_embed[bucket(d)][h]: the one table the attention reads
        const std::vector<float>& emb = vec("encoder.layers.0.attention.rel_attn_embed.weight");
        const int heads = g->cfg.num_attention_heads, W = 2 * g->max_distance + 1;
        std::vector<float> table((size_t)heads * W);
        for (int hd = 0; hd < heads; ++hd)
            for (int i = 0; i < W; ++i) table[(size_t)hd * W + i] = emb[(size_t)g->bucket_of[(size_t)i] * heads + hd];
        if ((rc = upload(h, table, &g->d_bias)) != HIFICAR_OK) return rc;
        HIP_TRY(hipFuncSetAttribute(x3 ? reinterpret_cast<const void*>(&hubert_attn_kernel<kHubHeadDim, true, true>)
                                       : reinterpret_cast<const void*>(&hubert_attn_kernel<kHubHeadDim, false, true>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)HubertAttnLds<kHubHeadDim, true>::bytes));
    } else if (g->precision == HIFICAR_PREC_BF16X3A) HIP_TRY(hubert_attn16_attr<kHubHeadDim>());
    else
        HIP_TRY(hipFuncSetAttribute(x3 ? reinterpret_cast<const void*>(&hubert_attn_kernel<kHubHeadDim, true>)
                                       : reinterpret_cast<const void*>(&hubert_attn_kernel<kHubHeadDim>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)HubertAttnLds<kHubHeadDim>::bytes));
    HIP_TRY(hubert_by_group(G, [](auto Gc) {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(&hubert_posconv_kernel<Gc()>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)HubertPosLds<Gc()>::bytes);
    }));
    // the engine opens here, not in hificar_hubert_create: a handle can be created and described without a device
    if ((rc = engine_open(h, true)) != HIFICAR_OK) return rc;
    h->precision = x3 ? HIFICAR_PREC_BF16X3 : HIFICAR_PREC_F32;
    h->use_pair = false;
    h->ksplit = 0;  // one accumulation order for every launch shape: an utterance's states do not depend on what it is batched with
    HIP_TRY(hipDeviceSynchronize());
    g->weights.clear_staged();
    g->finalized = true;
    return HIFICAR_OK;
}

// (bf16x3: the same buffers and bytes — a split row takes its fp32 row's bytes)
struct HubertWorkspace {
    double* stats;  // [B][mean, rstd]
    int* frames;    // [B]
    float* ea;      // extractor sub-batch: [Bs][P0][C] (layers 0, 2, 4, 6; bf16x3: every layer's split window rows)
    float* eb;      // [Bs][P1][C] (layers 1, 3, 5; bf16x3: every conv's fp32 rows)
    float* feat;    // [M][C]: layer 6's rows of the whole batch, then their LayerNorm (bf16x3: as split rows)
    float* r[4];    // [M][H]
    float* wide;    // [M][max(3 H, I)]
    float* gates;   // rel_bias: [B][heads][T], one layer's, reused by the next (null without)
    int Bs;         // utterances per extractor sub-batch
    size_t bytes;
};

static bool hubert_shape_ok(const hificar_hubert* g, int B, int L, HubertDims* d) {
    if (B < 1 || B > 65535 || !hubert_dims(L, d)) return false;
    const long long wide = std::max(3 * g->cfg.hidden_size, g->cfg.intermediate_size);
    if ((long long)d->P[0] * g->cfg.conv_dim > (1LL << 28)) return false;          // one utterance's layer-0 rows: 1 GiB
    if ((long long)B * d->T[6] * wide >= (1LL << 31)) return false;
    return true;
}

static HubertWorkspace hubert_plan_workspace(const hificar_hubert* g, int B, const HubertDims& d, void* base) {
    const size_t C = (size_t)g->cfg.conv_dim, H = (size_t)g->cfg.hidden_size, W = (size_t)std::max(3 * g->cfg.hidden_size, g->cfg.intermediate_size);
    HubertWorkspace w;
    const size_t per = (size_t)d.P[0] * C * sizeof(float);
    w.Bs = (int)std::min<size_t>((size_t)B, g->sub_batch > 0 ? (size_t)g->sub_batch : std::max<size_t>(1, kHubExtBudget / per));
    const size_t M = round_up_sz((size_t)B * (size_t)d.T[6] + 64, 256);  // whole tiles of slack behind the last row
    Carver cv(base, 256);
    w.stats = cv.take<double>((size_t)B * 2 * sizeof(double));
    w.frames = cv.take<int>((size_t)B * sizeof(int));
    w.ea = cv.floats(((size_t)w.Bs * d.P[0] + 256) * C);
    w.eb = cv.floats(((size_t)w.Bs * d.P[1] + 256) * C);
    w.feat = cv.floats(M * C);
    for (int i = 0; i < 4; ++i) w.r[i] = cv.floats(M * H);
    w.wide = cv.floats(M * W);
    // (the gates only: the (heads, T, T) bias never exists)
    w.gates = g->rel_bias ? cv.floats((size_t)B * (size_t)g->cfg.num_attention_heads * (size_t)d.T[6]) : nullptr;
    w.bytes = cv.bytes();
    return w;
}

extern "C" size_t hificar_hubert_workspace_bytes(const hificar_hubert* g, int B, int L) {
    HubertDims d;
    if (!g || !hubert_shape_ok(g, B, L, &d)) return 0;
    return hubert_plan_workspace(g, B, d, nullptr).bytes;
}

extern "C" int hificar_hubert_debug_sub_batch(hificar_hubert* g, int utterances) {
    if (!g || utterances < 0) return fail(HIFICAR_E_INVALID, "hificar_hubert_debug_sub_batch: null handle or a negative count");
    g->sub_batch = utterances;
    return HIFICAR_OK;
}

extern "C" int hificar_hubert_debug_tap(hificar_hubert* g, const char* name, float* dst, size_t capacity) {
    if (!g) return fail(HIFICAR_E_INVALID, "null handle");
    if (name && dst && hubert_x3(g) && std::string(name) == "extractor.0")
        return fail(HIFICAR_E_STATE, "debug tap 'extractor.0': a %s handle holds layer 0's rows as split bf16 window rows only, not as fp32 rows",
                    xfmr_precision_name(g->precision));
    g->taps.set(name, dst, capacity);
    return HIFICAR_OK;
}

// rows [nseq][rows][width] of a buffer with `pitch` rows per sequence -> the tap's dense (.., rows, width) at sequence `seq0`
static int hubert_emit_tap(hificar_hubert* g, const std::string& name, const float* src, int seq0, int nseq, int total_seq, size_t rows, size_t pitch,
                           size_t width, hipStream_t stream) {
    float* dst;
    const int rc = g->taps.find(name, (size_t)total_seq * rows * width, &dst);
    if (rc != HIFICAR_OK || !dst) return rc;
    HIP_TRY(hipMemcpy2DAsync(dst + (size_t)seq0 * rows * width, rows * width * sizeof(float), src, pitch * width * sizeof(float),
                             rows * width * sizeof(float), (size_t)nseq, hipMemcpyDeviceToDevice, stream));
    return HIFICAR_OK;
}

extern "C" int hificar_hubert_forward(hificar_hubert* g, const float* wav, const int32_t* lengths, const int32_t* lengths_host, float* out, int B, int L,
                                      int layer, void* workspace, size_t workspace_bytes, void* stream_) {
    if (!g || !wav || !out) return fail(HIFICAR_E_INVALID, "hificar_hubert_forward: null argument");
    if (L < HIFICAR_HUBERT_MIN_SAMPLES)
        return fail(HIFICAR_E_INVALID, "hificar_hubert_forward: L=%d: an utterance under %d samples has no frame", L, HIFICAR_HUBERT_MIN_SAMPLES);
    HubertDims d;
    if (!hubert_shape_ok(g, B, L, &d))
        return fail(HIFICAR_E_INVALID, "hificar_hubert_forward: B=%d, L=%d out of range (B <= 65535, B frames max(3 hidden, intermediate) < 2^31)", B, L);
    if (layer < -1 || layer >= g->cfg.num_hidden_layers)
        return fail(HIFICAR_E_INVALID, "hificar_hubert_forward: layer=%d outside -1 .. %d", layer, g->cfg.num_hidden_layers - 1);
    if (lengths_host && !lengths) return fail(HIFICAR_E_INVALID, "hificar_hubert_forward: lengths_host without the device copy");
    if (lengths_host)
        for (int b = 0; b < B; ++b)
            if (lengths_host[b] < HIFICAR_HUBERT_MIN_SAMPLES || lengths_host[b] > L)
                return fail(HIFICAR_E_INVALID, "hificar_hubert_forward: lengths[%d]=%d outside %d .. L=%d", b, lengths_host[b], HIFICAR_HUBERT_MIN_SAMPLES, L);
    const HubertWorkspace ws = hubert_plan_workspace(g, B, d, workspace);
    int rc;
    if ((rc = check_workspace(nullptr, workspace, workspace_bytes, ws.bytes)) != HIFICAR_OK) return rc;
    if (!g->finalized) return fail(HIFICAR_E_STATE, "hificar_hubert_forward before hificar_hubert_finalize");
    hificar_engine* h = &g->eng;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if ((rc = enter_stream(h, stream)) != HIFICAR_OK) return rc;
    const hificar_hubert_config& c = g->cfg;
    const int C = c.conv_dim, H = c.hidden_size, I = c.intermediate_size, T = d.T[6];
    const double M = (double)B * T;
    const bool x3 = hubert_x3(g), a16 = g->precision == HIFICAR_PREC_BF16X3A;
    // (a tap set before hificar_hubert_set_precision)
    if (x3 && g->taps.wanted("extractor.0"))
        return fail(HIFICAR_E_STATE, "debug tap 'extractor.0': a %s handle holds layer 0's rows as split bf16 window rows only", xfmr_precision_name(g->precision));

    if (c.normalize) {
        ProfScope prof(h, stream, "hubert_stats_kernel", 0.0, 8.0 * B * L);
        hipLaunchKernelGGL(hubert_stats_kernel, dim3((unsigned)B), dim3(256), 0, stream, wav, lengths, ws.stats, L, (double)c.norm_eps);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(hubert_frames_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, lengths, ws.frames, B, L);
    HIP_TRY(hipGetLastError());

    // split (bf16x3): dst takes split rows instead of fp32 rows — 1: rows of their own, 2: window rows of two positions (dst must not be src)
    auto layer_norm = [&](const float* src, const float* gamma, const float* beta, float* dst, int nseq, int rows, int rows_in, int rows_out, int F, float eps,
                          const int* lens, bool gelu, int split = 0, const HubertEncLayer* gate = nullptr) {
        HubertLnParams p;
        p.x = src;
        p.gamma = gamma;
        p.beta = beta;
        p.lengths = lens;
        p.y = dst;
        p.B = nseq;
        p.T = rows;
        p.Tin = rows_in;
        p.Tout = rows_out;
        p.F = F;
        p.eps = eps;
        p.window = split == 2;
        const double n = (double)nseq * rows;
        if (gate) {  // (a layer's first LayerNorm under rel_bias: no GELU, no window)
            p.gate_w = gate->d_gate[0];
            p.gate_b = gate->d_gate[1];
            p.gate_c = gate->d_gate[2];
            p.gates = ws.gates;
            ProfScope prof(h, stream, split ? "hubert_ln_kernel<gate,split>" : "hubert_ln_kernel<gate>", 8.0 * n * F + 2.0 * n * 8 * F, 8.0 * n * F);
            const dim3 grid((unsigned)(((long long)nseq * rows + 3) / 4));
            if (split) hipLaunchKernelGGL((hubert_ln_kernel<false, true, true>), grid, dim3(256), 0, stream, p);
            else hipLaunchKernelGGL((hubert_ln_kernel<false, false, true>), grid, dim3(256), 0, stream, p);
            return hipGetLastError();
        }
        ProfScope prof(h, stream, split ? (gelu ? "hubert_ln_kernel<gelu,split>" : "hubert_ln_kernel<split>") : gelu ? "hubert_ln_kernel<gelu>" : "hubert_ln_kernel",
                       8.0 * n * F, 8.0 * n * F);
        const dim3 grid((unsigned)(((long long)nseq * rows + 3) / 4));
        if (split && gelu) hipLaunchKernelGGL((hubert_ln_kernel<true, true>), grid, dim3(256), 0, stream, p);
        else if (split) hipLaunchKernelGGL((hubert_ln_kernel<false, true>), grid, dim3(256), 0, stream, p);
        else if (gelu) hipLaunchKernelGGL(hubert_ln_kernel<true>, grid, dim3(256), 0, stream, p);
        else hipLaunchKernelGGL(hubert_ln_kernel<false>, grid, dim3(256), 0, stream, p);
        return hipGetLastError();
    };

    // ---- the extractor, a sub-batch of utterances at a time
    for (int b0 = 0; b0 < B; b0 += ws.Bs) {
        const int nseq = std::min(ws.Bs, B - b0);
        {
            HubertConv0Params p;
            p.wav = wav + (size_t)b0 * L;
            p.lengths = lengths ? lengths + b0 : nullptr;
            p.stats = c.normalize ? ws.stats + 2 * (size_t)b0 : nullptr;
            p.w = g->d_w0;
            p.bias = g->d_b0;
            p.gamma = g->d_ext_ln[0][0];
            p.beta = g->d_ext_ln[0][1];
            p.y = ws.ea;
            p.nseq = nseq;
            p.L = L;
            p.T0 = d.T[0];
            p.P = d.P[0];
            p.C = C;
            const double n = (double)nseq * d.P[0];
            ProfScope prof(h, stream, x3 ? "hubert_conv0_kernel<split>" : "hubert_conv0_kernel", 2.0 * n * C * kHubK0, 4.0 * (n * C + (double)nseq * L));
            const dim3 grid((unsigned)(((long long)nseq * d.P[0] + 3) / 4));
            if (x3) hipLaunchKernelGGL(hubert_conv0_kernel<true>, grid, dim3(256), 0, stream, p);
            else hipLaunchKernelGGL(hubert_conv0_kernel<false>, grid, dim3(256), 0, stream, p);
            HIP_TRY(hipGetLastError());
        }
        if (!x3 && (rc = hubert_emit_tap(g, "extractor.0", ws.ea, b0, nseq, B, (size_t)d.T[0], (size_t)d.P[0], (size_t)C, stream)) != HIFICAR_OK) return rc;
        for (int i = 1; i < kHubExtLayers; ++i) {
            // (bf16x3: ws.ea holds every layer's split window rows, ws.eb every conv's fp32 rows)
            const float* const in = x3 || (i & 1) ? ws.ea : ws.eb;
            float* const y = x3 || (i & 1) ? ws.eb : ws.ea;
            ConvIO io{};
            io.xs = reinterpret_cast<const char*>(in);
            io.y = y;
            io.res = nullptr;
            io.ys = nullptr;
            io.x_seq_bytes = (long long)d.P[i - 1] * C * 4;  // rows of two positions: P / 2 windows of 2 C floats per sequence
            io.x_rows = d.P[i - 1] / 2;
            Ragged full;
            full.frames = d.P[i];
            if ((rc = launch_conv1(h, g->ext[i], nseq, d.P[i], io, 0.f, full, stream)) != HIFICAR_OK) return rc;
            const bool last = i + 1 == kHubExtLayers;
            HIP_TRY(layer_norm(y, g->d_ext_ln[i][0], g->d_ext_ln[i][1], last ? ws.feat + (size_t)b0 * T * C : x3 ? ws.ea : y, nseq, last ? T : d.P[i], d.P[i],
                               last ? T : d.P[i], C, 1e-5f, nullptr, true, x3 && !last ? 2 : 0));
        }
    }
    if ((rc = hubert_emit_tap(g, "extract_features", ws.feat, 0, B, B, (size_t)T, (size_t)T, (size_t)C, stream)) != HIFICAR_OK) return rc;

    // ---- everything at 50 Hz, under the ragged context
    Ragged rg;
    rg.seq_len = ws.frames;
    rg.frames = T;
    // xs: fp32 rows in exact fp32, split rows in bf16x3.  ys (bf16x3a's q | k | v): the output as split rows only — slope 1 makes the engine's
    // activated copy the identity
    auto conv = [&](const ConvLayer& Lr, const float* xs, const float* res, float* y, float* ys = nullptr) {
        ConvIO io{};
        io.xs = reinterpret_cast<const char*>(xs);
        io.res = res;
        io.y = y;
        io.ys = reinterpret_cast<char*>(ys);
        return launch_conv1(h, Lr, B, T, io, ys ? 1.f : 0.f, rg, stream);
    };
    const int sp = x3 ? 1 : 0;  // a LayerNorm in front of a GEMM writes that GEMM's operand
    auto tap = [&](const std::string& name, const float* rows) { return hubert_emit_tap(g, name, rows, 0, B, B, (size_t)T, (size_t)T, (size_t)H, stream); };
    HIP_TRY(layer_norm(ws.feat, g->d_fp_ln[0], g->d_fp_ln[1], ws.feat, B, T, T, T, C, c.layer_norm_eps, ws.frames, false, sp));
    if ((rc = conv(g->proj, ws.feat, nullptr, ws.r[0])) != HIFICAR_OK) return rc;
    if ((rc = tap("feature_projection", ws.r[0])) != HIFICAR_OK) return rc;
    float* cur = ws.r[1];    // the stream
    float* other = ws.r[0];  // ... and where the attention sub-block's sum goes
    float* const N = ws.r[2];
    float* const R = ws.r[3];
    {
        HubertPosParams p;
        p.x = ws.r[0];
        p.wp = g->d_pos_w;
        p.bias = g->d_pos_b;
        p.lengths = ws.frames;
        p.y = cur;
        p.pos_out = g->taps.wanted("pos_conv") ? N : nullptr;
        p.T = T;
        p.H = H;
        const int G = H / kHubPosGroups;
        ProfScope prof(h, stream, "hubert_posconv_kernel", 2.0 * M * H * G * kHubPosTaps, 4.0 * (2.0 * M * H + (double)H * G * kHubPosTaps));
        const dim3 grid((unsigned)((T + kHubPosTR - 1) / kHubPosTR), kHubPosGroups, (unsigned)B);
        const hipError_t e = hubert_by_group(G, [&](auto Gc) {
            hipLaunchKernelGGL(hubert_posconv_kernel<Gc()>, grid, dim3(256), HubertPosLds<Gc()>::bytes, stream, p);
            return hipGetLastError();
        });
        if (e != hipSuccess) return fail(HIFICAR_E_HIP, "hubert_posconv_kernel launch failed: %s", hipGetErrorString(e));
        if (p.pos_out && (rc = tap("pos_conv", N)) != HIFICAR_OK) return rc;
    }
    const int nrun = layer < 0 ? c.num_hidden_layers : layer;  // hidden_states[k] is the stream in front of layer k
    for (int l = 0; l < nrun; ++l) {
        const HubertEncLayer& E = g->enc[(size_t)l];
        HIP_TRY(layer_norm(cur, E.d_ln[0], E.d_ln[1], N, B, T, T, T, H, c.layer_norm_eps, ws.frames, false, sp, g->rel_bias ? &E : nullptr));
        if (g->rel_bias && (rc = hubert_emit_tap(g, "gate." + std::to_string(l), ws.gates, 0, B, B, (size_t)c.num_attention_heads,
                                                 (size_t)c.num_attention_heads, (size_t)T, stream)) != HIFICAR_OK)
            return rc;
        if ((rc = a16 ? conv(E.qkv, N, nullptr, nullptr, ws.wide) : conv(E.qkv, N, nullptr, ws.wide)) != HIFICAR_OK) return rc;
        if (a16) {
            HubertAttn16Params p;
            p.qkv = reinterpret_cast<const char*>(ws.wide);
            p.lengths = ws.frames;
            p.out = reinterpret_cast<char*>(R);
            p.T = T;
            p.F = H;
            p.scale = (float)(1.0 / std::sqrt((double)kHubHeadDim));
            ProfScope prof(h, stream, "hubert_attn16_kernel", 4.0 * M * T * H, 4.0 * M * 4 * H);
            const dim3 grid((unsigned)((T + kXfmrTQ - 1) / kXfmrTQ), (unsigned)c.num_attention_heads, (unsigned)B);
            hipLaunchKernelGGL(hubert_attn16_kernel<kHubHeadDim>, grid, dim3(256), HubertAttn16Lds<kHubHeadDim>::bytes, stream, p);
            HIP_TRY(hipGetLastError());
        } else {
            HubertAttnParams p;
            p.qkv = ws.wide;
            p.lengths = ws.frames;
            p.out = R;
            p.T = T;
            p.F = H;
            p.scale = (float)(1.0 / std::sqrt((double)kHubHeadDim));
            p.gates = ws.gates;
            p.bias = g->d_bias;
            p.maxd = g->max_distance;
            ProfScope prof(h, stream, g->rel_bias ? (x3 ? "hubert_attn_kernel<relbias,split>" : "hubert_attn_kernel<relbias>")
                                      : x3        ? "hubert_attn_kernel<split>"
                                                  : "hubert_attn_kernel",
                           4.0 * M * T * H, 4.0 * M * 4 * H);  // (every key of a full-length batch)
            const dim3 grid((unsigned)((T + kXfmrTQ - 1) / kXfmrTQ), (unsigned)c.num_attention_heads, (unsigned)B);
            // (bf16x3: the instantiation that stores split rows)
            constexpr size_t rel_lds = HubertAttnLds<kHubHeadDim, true>::bytes;
            if (g->rel_bias && x3) hipLaunchKernelGGL((hubert_attn_kernel<kHubHeadDim, true, true>), grid, dim3(256), rel_lds, stream, p);
            else if (g->rel_bias) hipLaunchKernelGGL((hubert_attn_kernel<kHubHeadDim, false, true>), grid, dim3(256), rel_lds, stream, p);
            else if (x3) hipLaunchKernelGGL((hubert_attn_kernel<kHubHeadDim, true>), grid, dim3(256), HubertAttnLds<kHubHeadDim>::bytes, stream, p);
            else hipLaunchKernelGGL(hubert_attn_kernel<kHubHeadDim>, grid, dim3(256), HubertAttnLds<kHubHeadDim>::bytes, stream, p);
            HIP_TRY(hipGetLastError());
        }
        if ((rc = conv(E.wo, R, cur, other)) != HIFICAR_OK) return rc;
        HIP_TRY(layer_norm(other, E.d_ln[2], E.d_ln[3], N, B, T, T, T, H, c.layer_norm_eps, ws.frames, false, sp));
        if ((rc = conv(E.l1, N, nullptr, ws.wide)) != HIFICAR_OK) return rc;
        if (x3) {
            ProfScope prof(h, stream, "hubert_gelu_split_kernel", 0.0, 8.0 * M * I);
            hipLaunchKernelGGL(hubert_gelu_split_kernel, dim3((unsigned)(B * T)), dim3(256), 0, stream, ws.wide, ws.frames, T, I);
            HIP_TRY(hipGetLastError());
        } else {
            ProfScope prof(h, stream, "hubert_gelu_kernel", 0.0, 8.0 * M * I);
            hipLaunchKernelGGL(hubert_gelu_kernel, dim3((unsigned)(B * T), (unsigned)((I / 4 + 255) / 256)), dim3(256), 0, stream, ws.wide, ws.frames, T, I);
            HIP_TRY(hipGetLastError());
        }
        if ((rc = conv(E.l2, ws.wide, other, cur)) != HIFICAR_OK) return rc;
        if ((rc = tap("layers." + std::to_string(l), cur)) != HIFICAR_OK) return rc;
    }
    const float* src = cur;
    if (layer < 0) {
        HIP_TRY(layer_norm(cur, g->d_enc_ln[0], g->d_enc_ln[1], N, B, T, T, T, H, c.layer_norm_eps, ws.frames, false));
        src = N;
    }
    {
        ProfScope prof(h, stream, "xfmr_out_kernel", 0.0, 8.0 * M * H);
        hipLaunchKernelGGL(xfmr_out_kernel, dim3((unsigned)((T + 31) / 32), (unsigned)(H / 32), (unsigned)B), dim3(256), 0, stream, src, out,
                           static_cast<const int*>(ws.frames), H, H, T, static_cast<const int*>(nullptr));
        HIP_TRY(hipGetLastError());
    }
    return HIFICAR_OK;
}
