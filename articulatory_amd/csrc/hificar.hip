// libhificar.so — host side of the C ABI declared in include/hificar.h.
// Builds the layer list of the reference's HiFiGANGenerator (articulatory/models/hifigan.py:108-175)
// from a hificar_config, repacks folded weights into the kernels' layouts, plans the workspace and
// enqueues the forward pass / the batched autoregressive loop on the caller's HIP stream.
#include "hificar_kernels.hip.h"
#include "hificar_launch.h"
#include "hificar_backward.hip.h"
#include "hificar_disc_kernels.hip.h"
#include "hificar_bigru_kernels.hip.h"
#include "hificar_bigru_train_kernels.hip.h"
#include "hificar_xfmr_kernels.hip.h"
#include "hificar_frontend_kernels.hip.h"
#include "hificar_feat_kernels.hip.h"
#include "hificar_xfmr_attn16.hip.h"
#include "hificar_xfmr_train_kernels.hip.h"
#include "hificar_xfmr_attn16_train.hip.h"
#include "hificar_xfmr_attn16_train_k.hip.h"
#include "hificar_xfmr_wgrad16.hip.h"
#include "hificar_hubert_kernels.hip.h"
#include "hificar_hubert_attn16.hip.h"

#include "../../include/hificar.h"

#include <algorithm>
#include <queue>
#include <set>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

using namespace hificar;

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[1024] = "";

static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t _e = (expr);                                                                     \
        if (_e != hipSuccess)                                                                       \
            return fail(HIFICAR_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

// ------------------------------------------------------------------------------------------------
// model description
// ------------------------------------------------------------------------------------------------
#include "hificar_host_util.h"  // HostTensor, Carver, WeightIntake, TapTable, check_workspace, launch_conv1, pack_linear

struct ConvLayer {
    std::string name;     // reference module path, e.g. "blocks.3.convs1.2.1"
    bool transposed = false;
    int cin = 0;          // real input channels
    int cin_pad = 0;      // row pitch of the input buffer (multiple of 16)
    int cout = 0;         // real output channels (per phase for transposed)
    int cout_pad = 0;     // output channels per phase as laid out in memory: cout rounded up to a multiple of 32 (extra channels have
                          // zero weights and bias, so they hold exact zeros through every layer and cost nothing in accuracy)
    int K = 0, dilation = 1, stride = 1, padding = 0;
    bool has_bias = true;
    // derived
    int n_phase = 1, ntaps = 0, cout_total = 0;
    int off_min = 0, off_max = 0;
    int tap_off[kMaxPhase][kMaxTaps];
    int tap_k[kMaxPhase][kMaxTaps];  // which kernel index each (phase, tap) uses; -1 = zero weights
    float* d_bias = nullptr;
    int chunk16 = 0, n_blocks32 = 0, nb32_per_phase = 0;
    uint16_t* d_w16 = nullptr;   // bf16x3 arithmetic: hi/lo bf16 weight fragments in MFMA lane order
    uint16_t* d_w16c = nullptr;  // same fragments packed with one K chunk = all channels (fused pair kernel, C <= 64)
    float* d_w32 = nullptr;      // exact-fp32 arithmetic: fp32 fragments in the same order
    float* d_w32c = nullptr;     // fp32 fragments with one K chunk = all channels (fused pair kernel, C <= 64)
};

// One GBlock of a GBlockGenerator (articulatory/layers/pytorch_layers.py:32-91): conv1 = [ReLU, Upsample, c1a, ReLU, c1b (dilation 3)],
// res1 = [Upsample, res (1 x 1)], conv2 = [ReLU, c2a (dilation 9), ReLU, c2b (dilation 27)]
struct GBlockLayers {
    ConvLayer c1a, c1b, res, c2a, c2b;
    int scale = 1;
    int cin = 0, cout = 0;
};

// A launch shape of the conv engine: what a ConvPlan is a function of, besides the engine's fixed switches.  A layer is identified by its
// address: every engine (generator, GBlock generator, their TrainState's data-gradient layers, the discriminators' per-group layers, mel)
// builds its ConvLayers once, in create / train_init, into storage it owns and never resizes afterwards.
struct PlanKey {
    const ConvLayer* layers[6];  // launch_conv: the branches' layers; launch_pair: conv1 of every branch, from [3] on conv2; null: no such branch
    int nseq, rows, zrep;
    int flags;                   // 1: exact fp32, 2: training (device-resident weights), 4: shared_chip, 8: launch_pair, 16: launch_merged (up to four layers)
    bool operator<(const PlanKey& o) const { return memcmp(this, &o, sizeof(PlanKey)) < 0; }  // (six pointers, four ints: no padding)
};

// Everything about a launch of launch_conv / launch_pair that its shape decides: computed on the first launch of that shape
// (build_conv_plan / build_pair_plan), looked up afterwards.
struct ConvPlan {
    ConvShape shape;
    unsigned grid = 0;
    size_t lds = 0;
    std::string name;  // kernel name for ProfScope ("kernel|layer xN" with profile_detail)
    // the kernel's parameter block with what the shape decides filled in — tile counts, LDS bytes, xcd_order, stage_cached and the plan's
    // own tile schedule in the arenas (null: the kernel's round-robin walk) — and the rest zero: a launch copies it and adds the call's IO
    MultiConvParams conv = {};  // launch_conv
    PairParams pair = {};       // launch_pair
    MergeConvParams merge = {}; // launch_merged
    bool merge_wins = false;    // launch_merged: the estimate puts this launch + a one-stream upsampler ahead of the side-by-side launch + the folded mean
};

// The conv engine: everything a launch needs whatever network owns it.  Every model type holds one — the generators by inheritance
// (hificar_handle below), hificar_disc / hificar_mel / hificar_bigru as a member — opened by engine_open, closed by engine_close.
struct hificar_engine {
    int precision = HIFICAR_PREC_F32;
    int num_cus = 256;
    bool training = false;         // weights are device-resident (the generator sets it where it creates its TrainState): part of the plan key
    bool profile_detail = false;   // HIFICAR_PROFILE_DETAIL=1: profile rows carry the layer name
    bool use_pair = true;          // HIFICAR_PAIR=0: layer by layer, no fused launch forms (neither the pair kernels nor the branch-summing launch)
    bool pair_small = true;        // HIFICAR_PAIR_SMALL: 128-row fused pair tiles at C = 32 for mid-size launches (pair_small_tiles)
    int mrf_merge = 1;             // HIFICAR_MRF_MERGE: 0 = never sum the MRF branches in the last ResBlock launch, 1 = where estimated faster (default), 2 = wherever allowed
    int ksplit = 1;                // HIFICAR_KSPLIT: 0 = never use the split-K conv form, 1 = when it is estimated faster (default), 2 = always
    double mi1_penalty = 1.05;     // cost factor of 32-row tiles in the exact-fp32 tile choice (they re-stream the weights most often: L2-bound when
                                   // K is long).  The discriminator engine raises it: its launches overlap on several streams, so a nearly
                                   // empty last round of taller tiles costs little there, while the L2 traffic of short tiles is shared by all
    int pick_throughput = 0;       // > 0: launches of at least this many tiles choose their tile shape by workgroup-time instead of makespan (set by
                                   // the discriminator engine, whose sub-networks run on eight streams; 0 = off)
    bool shared_chip = false;      // set while hificar_ar_loop runs two halves of a batch on two streams (launch_conv's tile choice)
    int force_tile[5] = {0, 0, 0, 0, 0};  // hificar_debug_force_tile: {MI, WM, WN, KS, NB} every launch_conv launch takes where it is admissible (MI = 0: none)
    std::vector<void*> allocs;     // device memory the engine's owner uploaded through it (upload, pack_w16 / pack_w32): freed by engine_close
    char* d_zeros = nullptr;       // 256 bytes of zeros: source of padding rows for the LDS DMA
    // launch plans, one per launch shape (get_plan), each with the tile schedule it built.  The schedules live in append-only arenas: a
    // device block plus a pinned host mirror, filled on the host and uploaded with ONE hipMemcpyAsync on the launch stream, so the first use of
    // a new launch shape neither allocates nor synchronises (the first arena is allocated by engine_open).  Dropped only together: evict_plans
    std::map<PlanKey, ConvPlan> plans;
    struct Arena {
        char* d = nullptr;
        char* h = nullptr;
        size_t cap = 0, used = 0;
    };
    std::vector<Arena> arenas;
    unsigned long long sched_up_seq = 0;  // schedule uploads so far (upload_schedule): a schedule is uploaded on the stream that first needs it
    // device copies of the batched-reduction tables of the backward passes (flush_reduce, hificar_train.hip.inc), cached by content: in steady
    // state a training iteration re-uses the tables of the iteration before (same buffers from the caller's caching allocator) without any upload
    struct ReduceSlot {
        char* d = nullptr;
        char* h = nullptr;
        size_t bytes = 0;
        unsigned long long hash = 0, stamp = 0;
        hipEvent_t ev = nullptr;  // recorded behind the last launch that reads the slot
        hipEvent_t up = nullptr;  // recorded behind the upload
        hipStream_t up_stream = nullptr;
    };
    std::vector<ReduceSlot> rslots;
    unsigned long long rstamp = 0;
    // every call's work is ordered behind the previous call's even when the caller switches streams (the schedules and, for a generator,
    // the packed step table and the workspace are shared state)
    hipStream_t last_stream = nullptr;
    bool have_last_stream = false;
    hipEvent_t xstream_ev = nullptr;
    hipEvent_t done_ev = nullptr;  // recorded at the END of the last call on done_stream (calls that mark their end: the discriminators' backward)
    bool done_valid = false;
    hipStream_t done_stream = nullptr;
    // profiling (hificar_profile_begin/end)
    bool profiling = false;
    struct ProfRec {
        hipEvent_t e0, e1;
        std::string name;
        double flops, bytes;
    };
    std::vector<ProfRec> prof;
    hipStream_t prof_stream = nullptr;
};

// The generator (HiFiGANGenerator or GBlockGenerator) on top of its engine: configuration, layers, AR step tables, taps, TrainState.
struct hificar_handle : hificar_engine {
    hificar_config cfg;
    int arch = 0;                  // 0: HiFiGANGenerator (hificar_create); 1: GBlockGenerator (hificar_gblock_create, hificar_gblock.hip.inc)
    std::vector<GBlockLayers> gb;  // arch 1
    int c_last = 0;                // channels in front of the output conv
    bool finalized = false;
    int cf = 0;       // feature channels = in_channels - ar_output*use_ar
    int cin_pad = 0;  // padded input-conv channels
    int hop = 1;
    WeightIntake weights;
    ConvLayer input_conv;
    std::vector<ConvLayer> ups;
    std::vector<ConvLayer> convs1;  // [stage][block][dil] flattened
    std::vector<ConvLayer> convs2;
    // output conv
    float* d_out_w = nullptr;
    float out_bias = 0.f;
    float* d_out_bias = nullptr;   // training (device-resident weights): the output conv's bias is read from here
    void* train = nullptr;         // TrainState (hificar_train.hip.inc), created by the first hificar_set_weight_device
    void (*train_free)(hificar_handle*) = nullptr;
    // MLP
    float* d_mlp_w[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    float* d_mlp_b[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    // speaker / phoneme conditioning
    float* d_spk_emb = nullptr;
    float* d_spk_w = nullptr;
    float* d_spk_b = nullptr;
    float* d_ph_emb = nullptr;
    float* d_phfc_w = nullptr;
    float* d_phfc_b = nullptr;
    void* d_tab = nullptr;    // step table of hificar_ar_loop_packed (grown on demand) and its pinned host staging copy
    void* h_tab = nullptr;
    size_t tab_bytes = 0;
    hipEvent_t tab_copied = nullptr;  // recorded behind the last upload: the staging copy may be rewritten once it has fired
    // step tables of hificar_ar_step: a ring of slots of mapped pinned host memory that front_kernel reads directly (no upload), one
    // per step in flight, each with the event recorded behind its step; a step only waits on the host when the ring has wrapped onto
    // a slot whose step is still queued.  step_d: the device copy front_kernel publishes for the step's later launches
    struct StepSlot {
        hipEvent_t done = nullptr;
        bool used = false;
    };
    std::vector<StepSlot> step_ring;
    char* step_d = nullptr;
    char* step_h = nullptr;
    char* step_hd = nullptr;  // step_h as the device sees it
    size_t step_cap = 0;      // table entries per slot
    unsigned step_next = 0;
    // AR loop of a small batch on two streams (hificar_ar_loop_ragged): the second stream, fork / join / schedule-upload events
    int ar_dual_min = 17, ar_dual_max = 62;  // HIFICAR_AR_DUAL_MIN / _MAX: the batch sizes the loop splits (max 0: never)
    hipStream_t ar_side = nullptr;
    hipEvent_t ar_ev[2] = {nullptr, nullptr};
    // debug taps (hificar_debug_tap); scratch for pre-activation copies
    TapTable taps;
    float* tap_scratch = nullptr;
    size_t tap_scratch_elems = 0;
};

// The library's environment switches — all of them.  engine_open reads the engine's own, once per engine: the generators' (in hificar_finalize),
// the discriminators' and the BiGRU's; the mel / STFT loss engine runs with the defaults.
//   HIFICAR_PROFILE_DETAIL=1   rows of hificar_profile_end carry the layer name ("kernel|layer xN"); weight-gradient rows the instantiation launched,
//                              the layer's shape, split count, row split and layers per launch ("wgrad_taps_kernel<7,0,128> 48x48k5p1 s3 r1 n2"),
//                              reduction rows which reduction ran ("wreduce_kernel ..", "wreduce_gemm_kernel<5> ..", "reduce_multi_kernel w9 b8")
//   HIFICAR_LAUNCH_LOG=<path>  every kernel launch of the library is appended to <path> in enqueue order as "kernel|layer<TAB>flops<TAB>algorithmic bytes":
//                              joined with rocprofv3's per-dispatch rows by tools/pmc_by_layer.py (implies PROFILE_DETAIL)
//   HIFICAR_KSPLIT=0|1|2       split-K conv form: never / when estimated faster (default) / always.  0 makes every launch shape use one accumulation
//                              order, so results are bit-identical across batch compositions (tests/test_gpu_parity.py)
//   HIFICAR_PAIR=0             layer by layer, no fused launch forms: neither the fused pair kernels of the narrow stages nor the branch-summing last
//                              ResBlock launch (one "layer xN" row per layer in the profile);  HIFICAR_PAIR_SMALL=0: no 128-row pair tiles at C = 32
//                              (the GBlock generator, the discriminators and the BiGRU have no such stages: they switch the pair kernels off)
//   HIFICAR_MRF_MERGE=0|1|2    the last ResBlock launch of a stage sums all blocks in one accumulator and writes the activated MRF mean (conv_f32mrg_kernel,
//                              exact fp32 inference only; mrf_merge_allowed): never / where the planner estimates it faster (default) / wherever allowed.
//                              Always off with HIFICAR_KSPLIT=0 (whether it runs depends on the launch size, and it rounds differently), HIFICAR_KSPLIT=2
//                              (the form is dense) and HIFICAR_PAIR=0.  A forced tile shape (hificar_debug_force_tile) does not enter the planner's estimate
// The generators add HIFICAR_AR_DUAL_MIN / _MAX: the batch sizes hificar_ar_loop runs as two halves on two streams (default 17..62; MAX=0: never).
// hificar_disc.hip.inc adds HIFICAR_DISC_STREAMS=0 (sub-discriminators on the caller's stream: per-launch counters) and HIFICAR_COL2IM_VEC4=0.
// hificar_bigru.hip.inc adds HIFICAR_BIGRU_NS=1|2 (sequences per workgroup of the recurrent kernel, A/B runs) and always runs with KSPLIT off.
// hificar_xfmr.hip.inc (the Transformer) adds none and always runs with KSPLIT off and without the pair kernels; so does hificar_hubert.hip.inc.
static FILE* g_launch_log = nullptr;
static void read_env_switches(hificar_engine* h) {
    if (const char* e = getenv("HIFICAR_PROFILE_DETAIL")) h->profile_detail = atoi(e) != 0;
    if (const char* e = getenv("HIFICAR_LAUNCH_LOG")) {
        if (!g_launch_log && *e) g_launch_log = fopen(e, "a");
        if (g_launch_log) h->profile_detail = true;
    }
    if (const char* e = getenv("HIFICAR_KSPLIT")) h->ksplit = atoi(e);
    if (const char* e = getenv("HIFICAR_PAIR")) h->use_pair = atoi(e) != 0;
    if (const char* e = getenv("HIFICAR_PAIR_SMALL")) h->pair_small = atoi(e) != 0;
    if (const char* e = getenv("HIFICAR_MRF_MERGE")) h->mrf_merge = atoi(e);
}

// RAII bracket around one kernel launch: the launch log, and an event before and after while profiling is on.
struct ProfScope {
    hificar_engine* h;
    hipStream_t s;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    std::string name;
    double flops, bytes;
    ProfScope(hificar_engine* h_, hipStream_t s_, const std::string& n, double f, double b) : h(h_), s(s_), flops(f), bytes(b) {
        if (g_launch_log) {
            fprintf(g_launch_log, "%s\t%.0f\t%.0f\n", n.c_str(), f, b);
            fflush(g_launch_log);
        }
        if (!h->profiling) return;
        name = n;
        (void)hipEventCreate(&e0);
        (void)hipEventCreate(&e1);
        (void)hipEventRecord(e0, s);
    }
    ~ProfScope() {
        if (!h->profiling) return;
        (void)hipEventRecord(e1, s);
        h->prof.push_back({e0, e1, name, flops, bytes});
        h->prof_stream = s;
    }
};

static size_t round_up_sz(size_t x, size_t m) { return (x + m - 1) / m * m; }
static int arena_add(hificar_engine* h, size_t min_bytes);
static void engine_close(hificar_engine* h);
static int bucket_frames(int T);

static int round_up(int x, int m) { return (x + m - 1) / m * m; }
static int stage_channels(const hificar_config& c, int i) { return c.channels >> i; }  // channels // 2**i
static int stage_pad(const hificar_config& c, int i) { return round_up(stage_channels(c, i), 32); }  // row pitch of that stage's buffers

static int conv_index(const hificar_handle* h, int stage, int block, int dil) {
    int idx = 0;
    for (int b = 0; b < stage * h->cfg.n_blocks + block; ++b) idx += h->cfg.n_dilations[b % h->cfg.n_blocks];
    return idx + dil;
}

// Derive tap tables and blocking for one layer.
static int plan_layer(ConvLayer& L) {
    if (L.cin_pad < 32 || L.cin_pad % 16 != 0 || L.cin < 1 || L.cout < 1)
        return fail(HIFICAR_E_INVALID, "internal: %s: bad channel counts (cin %d, padded %d, cout %d)", L.name.c_str(), L.cin, L.cin_pad, L.cout);
    L.cout_pad = round_up(L.cout, 32);  // any width runs (hifigan.py:108-145 accepts any): the MFMA tiles are 32 channels wide
    if (!L.transposed) {
        if (L.K > kMaxTaps) return fail(HIFICAR_E_INVALID, "%s: kernel size %d > %d", L.name.c_str(), L.K, kMaxTaps);
        L.n_phase = 1;
        L.ntaps = L.K;
        for (int k = 0; k < L.K; ++k) {
            L.tap_off[0][k] = k * L.dilation - L.padding;
            L.tap_k[0][k] = k;
        }
    } else {
        const int s = L.stride, p = L.padding;
        if (s > kMaxPhase) return fail(HIFICAR_E_INVALID, "%s: upsample scale %d > %d", L.name.c_str(), s, kMaxPhase);
        L.n_phase = s;
        L.ntaps = (L.K + s - 1) / s;
        if (L.ntaps > kMaxTaps) return fail(HIFICAR_E_INVALID, "%s: too many taps", L.name.c_str());
        for (int r = 0; r < s; ++r) {
            // out[q*s + r] = sum_k x[q + (r + p - k)/s] * W[:, :, k] over k == (r + p) mod s
            const int k0 = (r + p) % s;
            for (int t = 0; t < L.ntaps; ++t) {
                const int k = k0 + t * s;
                // (a tap past the kernel's end has zero weights; its offset continues the progression the K loop steps through)
                L.tap_k[r][t] = k < L.K ? k : -1;
                L.tap_off[r][t] = (r + p - k) / s;  // exact: r + p - k is a multiple of s
            }
        }
    }
    for (int r = 0; r < L.n_phase; ++r)
        for (int t = 1; t < L.ntaps; ++t)
            if (L.tap_off[r][t] - L.tap_off[r][t - 1] != L.tap_off[0][1] - L.tap_off[0][0])
                return fail(HIFICAR_E_INVALID, "%s: tap offsets are not an arithmetic progression", L.name.c_str());
    L.off_min = 0;
    L.off_max = 0;
    for (int r = 0; r < L.n_phase; ++r)
        for (int t = 0; t < L.ntaps; ++t) {
            L.off_min = std::min(L.off_min, L.tap_off[r][t]);
            L.off_max = std::max(L.off_max, L.tap_off[r][t]);
        }
    L.cout_total = L.cout_pad * L.n_phase;
    // 16/32/64 channels per LDS item (XOR-swizzled rows), and at least two items per tile (out-buffer hand-off)
    L.chunk16 = (L.cin_pad % 64 == 0 && L.cin_pad >= 128) ? 64 : (L.cin_pad % 32 == 0 && L.cin_pad >= 64) ? 32 : 16;
    L.n_blocks32 = L.cout_total / 32;
    L.nb32_per_phase = L.cout_pad / 32;
    return HIFICAR_OK;
}

// ------------------------------------------------------------------------------------------------
// create / destroy
// ------------------------------------------------------------------------------------------------
extern "C" const char* hificar_last_error(void) { return g_err; }
extern "C" const char* hificar_version(void) { return "hificar 0.1 gfx950"; }

extern "C" int hificar_create(const hificar_config* cfg, hificar_handle** out) {
    if (!cfg || !out) return fail(HIFICAR_E_INVALID, "hificar_create: null argument");
    const hificar_config& c = *cfg;
    if (c.out_channels != 1) return fail(HIFICAR_E_INVALID, "out_channels=%d unsupported (PQMF multi-band output is out of scope)", c.out_channels);
    if (c.kernel_size % 2 != 1) return fail(HIFICAR_E_INVALID, "Kernel size must be odd number.");
    if (c.n_stages < 1 || c.n_stages > HIFICAR_MAX_STAGES) return fail(HIFICAR_E_INVALID, "n_stages=%d out of range", c.n_stages);
    if (c.n_blocks < 1 || c.n_blocks > HIFICAR_MAX_BLOCKS)
        return fail(HIFICAR_E_INVALID, "n_blocks=%d unsupported (1..%d residual blocks per stage)", c.n_blocks, HIFICAR_MAX_BLOCKS);
    if (c.use_ar && (c.ar_input > 1024 || c.ar_hidden > 512 || c.ar_output > 512 || c.ar_input < 1))
        return fail(HIFICAR_E_INVALID, "PastFCEncoder: ar_input must be <= 1024, ar_hidden / ar_output <= 512");
    if (c.use_ar && (c.ar_hidden % 4 != 0 || c.ar_output % 4 != 0))
        return fail(HIFICAR_E_INVALID, "PastFCEncoder hidden/output dims must be multiples of 4");
    if (!(c.lrelu_slope >= 0.f && c.lrelu_slope <= 1.f)) return fail(HIFICAR_E_INVALID, "negative_slope=%g outside [0, 1]", c.lrelu_slope);
    if (c.precision != HIFICAR_PREC_F32 && c.precision != HIFICAR_PREC_BF16X3)
        return fail(HIFICAR_E_INVALID, "unknown precision %d", c.precision);
    if ((c.channels >> c.n_stages) < 1) return fail(HIFICAR_E_INVALID, "channels=%d leaves no channels after %d halvings", c.channels, c.n_stages);

    hificar_handle* h = new hificar_handle();
    h->cfg = c;
    h->precision = c.precision;
    if (c.use_spk_id && (c.num_spk < 1 || c.spk_emb_size < 1 || c.in_channels > 1024)) {
        delete h;
        return fail(HIFICAR_E_INVALID, "use_spk_id needs num_spk and spk_emb_size (and in_channels <= 1024)");
    }
    if ((c.use_ph || c.use_ph_loss) && c.num_ph < 1) {
        delete h;
        return fail(HIFICAR_E_INVALID, "use_ph / use_ph_loss need num_ph");
    }
    if (c.use_ph && c.ph_emb_size < 1) {
        delete h;
        return fail(HIFICAR_E_INVALID, "use_ph needs ph_emb_size");
    }
    if (c.use_spk_id && c.use_ph) {
        delete h;
        // spk_fc maps to in_channels values but is added before the phoneme channels are appended: the shapes disagree in the reference
        return fail(HIFICAR_E_INVALID, "use_spk_id together with use_ph is ill-formed in the reference (hifigan.py:212-220)");
    }
    h->cf = c.in_channels - (c.use_ar ? c.ar_output : 0) - (c.use_ph ? c.ph_emb_size : 0);
    if (h->cf < 1) {
        delete h;
        return fail(HIFICAR_E_INVALID, "in_channels=%d leaves no feature channels", c.in_channels);
    }
    h->cin_pad = std::max(32, round_up(c.in_channels, 16));
    h->hop = 1;
    for (int i = 0; i < c.n_stages; ++i) h->hop *= c.upsample_scales[i];

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

    for (int i = 0; i < c.n_stages && rc == HIFICAR_OK; ++i) {
        const int s = c.upsample_scales[i], K = c.upsample_kernel_sizes[i];
        const int pad = s / 2 + s % 2, opad = s % 2;  // hifigan.py:82-103
        if (K - 2 * pad + opad != s) {
            rc = fail(HIFICAR_E_INVALID, "upsample stage %d: kernel %d / scale %d does not give L_out = scale*L_in", i, K, s);
            break;
        }
        ConvLayer u;
        u.name = "upsamples." + std::to_string(i) + ".1";
        u.transposed = true;
        u.cin = stage_channels(c, i);
        u.cin_pad = stage_pad(c, i);
        u.cout = stage_channels(c, i + 1);
        u.K = K;
        u.stride = s;
        u.padding = pad;
        rc = plan_layer(u);
        expect(u.name + ".weight", {u.cin, u.cout, K});
        expect(u.name + ".bias", {u.cout});
        h->ups.push_back(u);
        for (int j = 0; j < c.n_blocks && rc == HIFICAR_OK; ++j) {
            const int k = c.resblock_kernel_sizes[j];
            if (k % 2 != 1) {
                rc = fail(HIFICAR_E_INVALID, "Kernel size must be odd number.");
                break;
            }
            if (c.n_dilations[j] < 1 || c.n_dilations[j] > HIFICAR_MAX_DILATIONS) {
                rc = fail(HIFICAR_E_INVALID, "block %d: n_dilations out of range", j);
                break;
            }
            for (int d = 0; d < c.n_dilations[j] && rc == HIFICAR_OK; ++d) {
                const std::string base = "blocks." + std::to_string(i * c.n_blocks + j);
                ConvLayer c1;
                c1.name = base + ".convs1." + std::to_string(d) + ".1";
                c1.cin = c1.cout = u.cout;
                c1.cin_pad = stage_pad(c, i + 1);
                c1.K = k;
                c1.dilation = c.resblock_dilations[j][d];
                c1.padding = (k - 1) / 2 * c1.dilation;
                c1.has_bias = c.bias != 0;
                rc = plan_layer(c1);
                ConvLayer c2 = c1;
                c2.name = base + ".convs2." + std::to_string(d) + ".1";
                c2.dilation = 1;
                c2.padding = (k - 1) / 2;
                if (rc == HIFICAR_OK) rc = plan_layer(c2);
                // use_additional_convs = false (residual_block.py:151, 191-205): no convs2, a layer is x = x + conv1(LeakyReLU(x))
                for (const ConvLayer* l : {&c1, &c2}) {
                    if (l == &c2 && !c.use_additional_convs) continue;
                    expect(l->name + ".weight", {l->cout, l->cin, k});
                    if (l->has_bias) expect(l->name + ".bias", {l->cout});
                }
                h->convs1.push_back(c1);
                if (c.use_additional_convs) h->convs2.push_back(c2);
            }
        }
    }
    const int c_last = stage_channels(c, c.n_stages);
    h->c_last = c_last;
    expect("output_conv.1.weight", {1, c_last, c.kernel_size});
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
    if (c.use_ph) expect("ph_emb_mat.weight", {c.num_ph, c.ph_emb_size});
    if (c.use_ph_loss) {
        if (c_last > 128) rc = fail(HIFICAR_E_INVALID, "use_ph_loss: the phoneme head handles up to 128 last-stage channels (got %d)", c_last);
        if (h->hop % 2 != 0) rc = fail(HIFICAR_E_INVALID, "use_ph_loss: prod(upsample_scales) must be even (hifigan.py:186)");
        expect("ph_fc.weight", {c.num_ph, c_last});
        expect("ph_fc.bias", {c.num_ph});
    }
    if (rc != HIFICAR_OK) {
        delete h;
        return rc;
    }
    *out = h;
    return HIFICAR_OK;
}

extern "C" void hificar_destroy(hificar_handle* h) {
    if (!h) return;
    if (h->d_tab) (void)hipFree(h->d_tab);
    if (h->h_tab) (void)hipHostFree(h->h_tab);
    if (h->tap_scratch) (void)hipFree(h->tap_scratch);
    if (h->train_free) h->train_free(h);
    if (h->tab_copied) (void)hipEventDestroy(h->tab_copied);
    if (h->step_d) (void)hipFree(h->step_d);
    if (h->step_h) (void)hipHostFree(h->step_h);
    for (auto& st : h->step_ring)
        if (st.done) (void)hipEventDestroy(st.done);
    if (h->ar_side) (void)hipStreamDestroy(h->ar_side);
    for (hipEvent_t e : h->ar_ev)
        if (e) (void)hipEventDestroy(e);
    engine_close(h);
    delete h;
}

extern "C" int hificar_set_weight(hificar_handle* h, const char* name, const float* data, const int64_t* shape, int ndim) {
    if (!h || !name || !data || !shape) return fail(HIFICAR_E_INVALID, "hificar_set_weight: null argument");
    if (h->finalized) return fail(HIFICAR_E_STATE, "hificar_set_weight(%s) after hificar_finalize", name);
    return h->weights.set(name, data, shape, ndim);
}

// ------------------------------------------------------------------------------------------------
// finalize: repack + upload
// ------------------------------------------------------------------------------------------------
static int upload(hificar_engine* h, const std::vector<float>& v, float** dptr) {
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, std::max<size_t>(v.size(), 1) * sizeof(float)));
    h->allocs.push_back(p);
    HIP_TRY(hipMemcpy(p, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
    *dptr = static_cast<float*>(p);
    return HIFICAR_OK;
}

static inline uint16_t f32_to_bf16(float f) {  // round to nearest even (finite inputs)
    uint32_t u;
    memcpy(&u, &f, 4);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
static inline float bf16_to_f32(uint16_t b) {
    uint32_t u = (uint32_t)b << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// bf16x3 path: weight fragments in MFMA lane order, [n_block32][chunk][tap][c16][hi|lo][lane][8]
static int pack_w16(hificar_engine* h, const ConvLayer& L, const HostTensor& W, int chunk, uint16_t** out) {
    const int nc16 = chunk / 16, nchunk = L.cin_pad / chunk;
    const size_t frag = 64 * 8;  // bf16 elements per fragment
    std::vector<uint16_t> w16(((size_t)L.n_blocks32 * nchunk * L.ntaps * nc16 * 2 + 4 * nc16) * frag, 0);
    for (int nb = 0; nb < L.n_blocks32; ++nb) {
        const int phase = nb / L.nb32_per_phase;
        const int co0 = (nb % L.nb32_per_phase) * 32;
        for (int c = 0; c < nchunk; ++c)
            for (int t = 0; t < L.ntaps; ++t) {
                const int k = L.tap_k[phase][t];
                if (k < 0) continue;
                for (int u = 0; u < nc16; ++u) {
                    uint16_t* hi = &w16[(((((size_t)nb * nchunk + c) * L.ntaps + t) * nc16 + u) * 2) * frag];
                    uint16_t* lo = hi + frag;
                    for (int lane = 0; lane < 64; ++lane) {
                        const int g = lane >> 5, n = lane & 31, co = co0 + n;
                        if (co >= L.cout) continue;
                        for (int j = 0; j < 8; ++j) {
                            const int ci = c * chunk + u * 16 + 8 * g + j;
                            if (ci >= L.cin) continue;
                            const size_t src = L.transposed ? ((size_t)ci * L.cout + co) * L.K + k : ((size_t)co * L.cin + ci) * L.K + k;
                            const float v = W.data[src];
                            const uint16_t vh = f32_to_bf16(v);
                            hi[lane * 8 + j] = vh;
                            lo[lane * 8 + j] = f32_to_bf16(v - bf16_to_f32(vh));
                        }
                    }
                }
            }
    }
    void* dp = nullptr;
    HIP_TRY(hipMalloc(&dp, w16.size() * sizeof(uint16_t)));
    h->allocs.push_back(dp);
    HIP_TRY(hipMemcpy(dp, w16.data(), w16.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    *out = static_cast<uint16_t*>(dp);
    return HIFICAR_OK;
}

// exact-fp32 arithmetic: fp32 weight fragments, [n_block32][chunk][tap][c16][half][lane][4]: lane (n = lane & 31, g = lane >> 5)
// holds channels 16*c16 + 8*half + 4*g + {0..3} of output channel n (one v_mfma_f32_32x32x2_f32 step per element)
static int pack_w32(hificar_engine* h, const ConvLayer& L, const HostTensor& W, int chunk, float** out) {
    const int nc16 = chunk / 16, nchunk = L.cin_pad / chunk;
    const size_t frag = 64 * 4;  // floats per fragment
    std::vector<float> w32(((size_t)L.n_blocks32 * nchunk * L.ntaps * nc16 * 2 + 4 * nc16) * frag, 0.f);
    for (int nb = 0; nb < L.n_blocks32; ++nb) {
        const int phase = nb / L.nb32_per_phase;
        const int co0 = (nb % L.nb32_per_phase) * 32;
        for (int c = 0; c < nchunk; ++c)
            for (int t = 0; t < L.ntaps; ++t) {
                const int k = L.tap_k[phase][t];
                if (k < 0) continue;
                for (int u = 0; u < nc16; ++u)
                    for (int v = 0; v < 2; ++v) {
                        float* f = &w32[((((((size_t)nb * nchunk + c) * L.ntaps + t) * nc16 + u) * 2) + v) * frag];
                        for (int lane = 0; lane < 64; ++lane) {
                            const int g = lane >> 5, n = lane & 31, co = co0 + n;
                            if (co >= L.cout) continue;
                            for (int j = 0; j < 4; ++j) {
                                const int ci = c * chunk + u * 16 + 8 * v + 4 * g + j;
                                if (ci >= L.cin) continue;
                                const size_t src = L.transposed ? ((size_t)ci * L.cout + co) * L.K + k : ((size_t)co * L.cin + ci) * L.K + k;
                                f[lane * 4 + j] = W.data[src];
                            }
                        }
                    }
            }
    }
    return upload(h, w32, out);
}

// W: the layer's folded weight; Bv: its bias (null: none, zeros are uploaded)
static int pack_conv(hificar_engine* h, ConvLayer& L, const HostTensor& W, const HostTensor* Bv) {
    std::vector<float> bias((size_t)L.cout_total, 0.f);
    for (int r = 0; Bv && r < L.n_phase; ++r)
        for (int co = 0; co < L.cout; ++co) bias[(size_t)r * L.cout_pad + co] = Bv->data[co];
    int rc = upload(h, bias, &L.d_bias);
    if (rc != HIFICAR_OK) return rc;

    if ((rc = pack_w16(h, L, W, L.chunk16, &L.d_w16)) != HIFICAR_OK) return rc;
    if ((rc = pack_w32(h, L, W, L.chunk16, &L.d_w32)) != HIFICAR_OK) return rc;
    if (!L.transposed && L.cin_pad == L.cin && (L.cin == 32 || L.cin == 64) && L.cout == L.cin) {
        if ((rc = pack_w16(h, L, W, L.cin_pad, &L.d_w16c)) != HIFICAR_OK) return rc;
        if ((rc = pack_w32(h, L, W, L.cin_pad, &L.d_w32c)) != HIFICAR_OK) return rc;
    }
    return HIFICAR_OK;
}

// the conv kernels' instantiation sets (hificar_conv_inst.hip): the one place the host code meets them
hipError_t hificar::conv_launch(const ConvShape& s, const void* params, dim3 grid, size_t lds_bytes, hipStream_t stream) {
    bool handled = false;
    hipError_t e = hipSuccess;
#define HIFICAR_TRY_SET(n)                                                      \
    if (!handled) e = conv_inst_launch_##n(s, params, grid, lds_bytes, stream, &handled); \
    if (handled) return e;
    HIFICAR_TRY_SET(0) HIFICAR_TRY_SET(1) HIFICAR_TRY_SET(2) HIFICAR_TRY_SET(3) HIFICAR_TRY_SET(4)
    HIFICAR_TRY_SET(5) HIFICAR_TRY_SET(6) HIFICAR_TRY_SET(7) HIFICAR_TRY_SET(8) HIFICAR_TRY_SET(9)
    HIFICAR_TRY_SET(10) HIFICAR_TRY_SET(11) HIFICAR_TRY_SET(12)
#undef HIFICAR_TRY_SET
    return hipErrorInvalidValue;  // a shape that is not built
}

hipError_t hificar::conv_set_lds_attributes() {
    hipError_t e = hipSuccess;
#define HIFICAR_ATTR_SET(n) \
    if (e == hipSuccess) e = conv_inst_attrs_##n();
    HIFICAR_ATTR_SET(0) HIFICAR_ATTR_SET(1) HIFICAR_ATTR_SET(2) HIFICAR_ATTR_SET(3) HIFICAR_ATTR_SET(4)
    HIFICAR_ATTR_SET(5) HIFICAR_ATTR_SET(6) HIFICAR_ATTR_SET(7) HIFICAR_ATTR_SET(8) HIFICAR_ATTR_SET(9)
    HIFICAR_ATTR_SET(10) HIFICAR_ATTR_SET(11) HIFICAR_ATTR_SET(12)
#undef HIFICAR_ATTR_SET
    return e;
}

// Opens an engine: the chip's size, the environment switches (read_env; its owner's overrides come after), and the device-side state every
// launch needs — the zero page of the LDS DMA, the kernels' dynamic-LDS attributes, the first schedule arena.
static int engine_open(hificar_engine* h, bool read_env) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
        h->num_cus = prop.multiProcessorCount;
    if (read_env) read_env_switches(h);
    void* z = nullptr;
    HIP_TRY(hipMalloc(&z, 256));
    h->allocs.push_back(z);
    HIP_TRY(hipMemset(z, 0, 256));
    h->d_zeros = static_cast<char*>(z);
    HIP_TRY(conv_set_lds_attributes());
    return h->arenas.empty() ? arena_add(h, 0) : HIFICAR_OK;
}

// Frees what the engine owns (opened or not: uploads may precede engine_open).
static void engine_close(hificar_engine* h) {
    for (void* p : h->allocs) (void)hipFree(p);
    for (auto& a : h->arenas) {
        (void)hipFree(a.d);
        (void)hipHostFree(a.h);
    }
    if (h->xstream_ev) (void)hipEventDestroy(h->xstream_ev);
    if (h->done_ev) (void)hipEventDestroy(h->done_ev);
    for (auto& r : h->rslots) {
        if (r.d) (void)hipFree(r.d);
        if (r.h) (void)hipHostFree(r.h);
        if (r.ev) (void)hipEventDestroy(r.ev);
        if (r.up) (void)hipEventDestroy(r.up);
    }
    for (auto& r : h->prof) {
        (void)hipEventDestroy(r.e0);
        (void)hipEventDestroy(r.e1);
    }
}

extern "C" int hificar_finalize(hificar_handle* h) {
    if (!h) return fail(HIFICAR_E_INVALID, "hificar_finalize: null handle");
    if (h->finalized) return HIFICAR_OK;
    if (const int missing = h->weights.check_complete()) return missing;
    int rc;
    auto pack = [&](ConvLayer& L) { return pack_conv(h, L, h->weights.at(L.name + ".weight"), L.has_bias ? &h->weights.at(L.name + ".bias") : nullptr); };
    if ((rc = pack(h->input_conv)) != HIFICAR_OK) return rc;
    for (auto& l : h->ups)
        if ((rc = pack(l)) != HIFICAR_OK) return rc;
    for (auto& l : h->convs1)
        if ((rc = pack(l)) != HIFICAR_OK) return rc;
    for (auto& l : h->convs2)
        if ((rc = pack(l)) != HIFICAR_OK) return rc;
    for (auto& g : h->gb)
        for (ConvLayer* l : {&g.c1a, &g.c1b, &g.res, &g.c2a, &g.c2b})
            if ((rc = pack(*l)) != HIFICAR_OK) return rc;
    {   // output conv weight (1, C, K) -> [k][C]
        const HostTensor& W = h->weights.at("output_conv.1.weight");
        const int C = (int)W.shape[1], K = (int)W.shape[2], Cp = round_up(C, 32);  // [k][padded channels]
        std::vector<float> w((size_t)Cp * K, 0.f);
        for (int ch = 0; ch < C; ++ch)
            for (int k = 0; k < K; ++k) w[(size_t)k * Cp + ch] = W.data[(size_t)ch * K + k];
        if ((rc = upload(h, w, &h->d_out_w)) != HIFICAR_OK) return rc;
        h->out_bias = h->weights.data("output_conv.1.bias")[0];
    }
    if (h->cfg.use_ar) {
        for (int l = 0; l < 5; ++l) {
            const HostTensor& W = h->weights.at("ar_model.model." + std::to_string(2 * l) + ".weight");
            const int dout = (int)W.shape[0], din = (int)W.shape[1];
            std::vector<float> wt((size_t)din * dout);
            for (int o = 0; o < dout; ++o)
                for (int i = 0; i < din; ++i) wt[(size_t)i * dout + o] = W.data[(size_t)o * din + i];
            if ((rc = upload(h, wt, &h->d_mlp_w[l])) != HIFICAR_OK) return rc;
            if ((rc = upload(h, h->weights.data("ar_model.model." + std::to_string(2 * l) + ".bias"), &h->d_mlp_b[l])) != HIFICAR_OK) return rc;
        }
    }
    if (h->cfg.use_spk_id) {
        if ((rc = upload(h, h->weights.data("spk_emb_mat.weight"), &h->d_spk_emb)) != HIFICAR_OK) return rc;
        if ((rc = upload(h, h->weights.data("spk_fc.weight"), &h->d_spk_w)) != HIFICAR_OK) return rc;
        if ((rc = upload(h, h->weights.data("spk_fc.bias"), &h->d_spk_b)) != HIFICAR_OK) return rc;
    }
    if (h->cfg.use_ph && (rc = upload(h, h->weights.data("ph_emb_mat.weight"), &h->d_ph_emb)) != HIFICAR_OK) return rc;
    if (h->cfg.use_ph_loss) {
        if ((rc = upload(h, h->weights.data("ph_fc.weight"), &h->d_phfc_w)) != HIFICAR_OK) return rc;
        if ((rc = upload(h, h->weights.data("ph_fc.bias"), &h->d_phfc_b)) != HIFICAR_OK) return rc;
    }
    // the engine opens here, not in hificar_create / hificar_gblock_create: a handle can be created and described without a device
    if ((rc = engine_open(h, true)) != HIFICAR_OK) return rc;
    if (h->arch == 1) h->use_pair = false;  // (the fused conv1 -> conv2 kernel is the HiFi-GAN ResBlock's)
    if (const char* e = getenv("HIFICAR_AR_DUAL_MIN")) h->ar_dual_min = atoi(e);
    if (const char* e = getenv("HIFICAR_AR_DUAL_MAX")) h->ar_dual_max = atoi(e);
    HIP_TRY(hipDeviceSynchronize());
    h->weights.clear_staged();  // host copies no longer needed
    h->finalized = true;
    return HIFICAR_OK;
}

extern "C" int hificar_set_precision(hificar_handle* h, int precision) {
    if (!h) return fail(HIFICAR_E_INVALID, "null handle");
    if (h->arch == 1 && precision != HIFICAR_PREC_F32)
        return fail(HIFICAR_E_INVALID, "GBlockGenerator runs in the exact-fp32 arithmetic only (its 1 x 1 residual conv reads raw, un-activated rows)");
    if (precision == HIFICAR_PREC_F32 || precision == HIFICAR_PREC_BF16X3) {
        h->precision = precision;
        return HIFICAR_OK;
    }
    return fail(HIFICAR_E_INVALID, "unknown precision %d", precision);
}

// ------------------------------------------------------------------------------------------------
// workspace plan
// ------------------------------------------------------------------------------------------------
constexpr int kMaxBlk = HIFICAR_MAX_BLOCKS;  // residual blocks per stage (hifigan.py:134-145: one per resblock_kernel_sizes entry)

struct Workspace {
    // "activated rows" = LeakyReLU(x) as split rows (bf16x3) or plain fp32 rows (exact fp32): 4 bytes per element either way
    float* xin;    // (B, T, cin_pad) assembled input rows (no activation in front of the input conv)
    float* h0;     // input conv output, activated rows
    float* u;      // upsample output, fp32 (residual of the first ResBlock layer)
    float* x[kMaxBlk];   // per-branch residual stream, fp32
    float* xt[kMaxBlk];  // conv1 output, activated rows ([0] also holds the activated MRF mean for the next upsampler)
    char* u_s;           // activated rows of u
    char* x_s[kMaxBlk];  // activated rows of x_j
    size_t bytes;
};

static size_t stage_elems(const hificar_handle* h, int B, int T) {
    size_t mx = 0, L = (size_t)T;
    if (h->arch == 1) {  // GBlockGenerator: the input conv's output and every GBlock's output live in stage buffers
        mx = L * (size_t)stage_pad(h->cfg, 0);
        for (const GBlockLayers& g : h->gb) {
            L *= (size_t)g.scale;
            mx = std::max(mx, L * (size_t)std::max(g.c1a.cin_pad, g.c1a.cout_pad));
        }
        return mx * (size_t)B;
    }
    for (int i = 0; i < h->cfg.n_stages; ++i) {
        L *= h->cfg.upsample_scales[i];
        mx = std::max(mx, L * (size_t)stage_pad(h->cfg, i + 1));
    }
    return mx * (size_t)B;
}

// One layout for both arithmetics (set_precision may switch a live handle).
static Workspace plan_workspace(const hificar_handle* h, int B, int T, void* base) {
    Workspace w;
    Carver cv(base, 1024);
    w.xin = cv.floats((size_t)B * T * h->cin_pad);
    w.h0 = cv.floats((size_t)B * T * stage_pad(h->cfg, 0));
    const size_t se = stage_elems(h, B, T);
    w.u = cv.floats(se);
    const int nbw = std::max(3, h->cfg.n_blocks);  // (three sets at least: the GBlock engine and the MRF-mean ping-pong use them by index)
    for (int j = 0; j < kMaxBlk; ++j) w.x[j] = j < nbw ? cv.floats(se) : nullptr;
    for (int j = 0; j < kMaxBlk; ++j) w.xt[j] = j < nbw ? cv.floats(se) : nullptr;
    w.u_s = cv.floats<char>(se);
    for (int j = 0; j < kMaxBlk; ++j) w.x_s[j] = j < nbw ? cv.floats<char>(se) : nullptr;
    w.bytes = cv.bytes();
    return w;
}

extern "C" size_t hificar_workspace_bytes(const hificar_handle* h, int B, int T) {
    if (!h || B < 1 || T < 1) return 0;
    const int Tb = bucket_frames(T);
    size_t n = plan_workspace(h, B, Tb, nullptr).bytes;
    if (B >= 2)  // room for the two halves of the batch side by side (hificar_ar_loop on two streams; buffer sizes round up to 1 KB)
        n = std::max(n, plan_workspace(h, (B + 1) / 2, Tb, nullptr).bytes + plan_workspace(h, B / 2, Tb, nullptr).bytes);
    return n;
}

extern "C" double hificar_macs(const hificar_handle* h, int B, int T) {
    if (!h) return 0.0;
    const hificar_config& c = h->cfg;
    double m = (double)T * c.in_channels * c.channels * c.kernel_size;
    double L = T;
    for (const GBlockLayers& g : h->gb) {  // arch 1: four k-tap convs and the 1 x 1 residual conv per output row
        L *= g.scale;
        m += L * ((double)g.cin * g.cout * (g.c1a.K + 1) + 3.0 * g.cout * g.cout * g.c1a.K);
    }
    if (h->arch == 1) {
        m += L * h->c_last * c.kernel_size;
        if (c.use_ar) m += (double)c.ar_input * c.ar_hidden + 3.0 * c.ar_hidden * c.ar_hidden + (double)c.ar_hidden * c.ar_output;
        return m * B;
    }
    for (int i = 0; i < c.n_stages; ++i) {
        const double cin = stage_channels(c, i), cout = stage_channels(c, i + 1);
        m += L * cin * cout * c.upsample_kernel_sizes[i];
        L *= c.upsample_scales[i];
        for (int j = 0; j < c.n_blocks; ++j) m += L * cout * cout * c.resblock_kernel_sizes[j] * (c.use_additional_convs ? 2.0 : 1.0) * c.n_dilations[j];
    }
    m += L * stage_channels(c, c.n_stages) * c.kernel_size;
    if (c.use_ar) m += (double)c.ar_input * c.ar_hidden + 3.0 * c.ar_hidden * c.ar_hidden + (double)c.ar_hidden * c.ar_output;
    return m * B;
}

// ------------------------------------------------------------------------------------------------
// launches
// ------------------------------------------------------------------------------------------------
// Training tape: every activated conv input of one forward gets its own buffer (the backward pass reads them: wgrad operands and
// LeakyReLU' masks); nothing is overwritten.  Filled by plan_tape() from a caller-provided tape buffer.
struct Tape {
    float* xin = nullptr;                                              // (B, T, cin_pad) assembled input rows
    char* h0_s = nullptr;                                              // activated input-conv output
    char* upin_s[HIFICAR_MAX_STAGES] = {};                             // activated input of upsample i (i = 0: h0_s)
    char* u_s[HIFICAR_MAX_STAGES] = {};                                // activated upsample output
    char* xt_s[HIFICAR_MAX_STAGES][kMaxBlk][HIFICAR_MAX_DILATIONS] = {};     // activated conv1 output (= conv2 input)
    char* x_s[HIFICAR_MAX_STAGES][kMaxBlk][HIFICAR_MAX_DILATIONS] = {};      // activated residual stream after pair d (= next conv1 input)
    float* mlp = nullptr;                                              // (B, 5, 1024) PastFCEncoder layer inputs
    float* fin[kMaxBlk] = {};                                          // fp32 ResBlock outputs of the LAST stage (output conv backward)
    // GBlockGenerator (arch 1), per GBlock: the raw and the ReLU'd input at the block's OUTPUT rate (nearest-upsampled copies: the weight
    // gradients of res1 / conv1's first conv contract over them), and the ReLU'd inputs of the other three convs
    char* g_xu[HIFICAR_MAX_GBLOCKS] = {};
    char* g_a1u[HIFICAR_MAX_GBLOCKS] = {};
    char* g_a2[HIFICAR_MAX_GBLOCKS] = {};
    char* g_a3[HIFICAR_MAX_GBLOCKS] = {};
    char* g_a4[HIFICAR_MAX_GBLOCKS] = {};
    size_t bytes = 0;
};

// One generator forward on B sequences of T frames, as its entry point describes it: every caller fills the fields it uses.
//   c: element (b, ch, t) at c[b*c_bstride + ch*c_cstride + t];  prev: (b, i) at prev[b*prev_bstride + i] or null
//   out: sample (b, n) at out[b*out_bstride + n]
struct FwdCall {
    const float* c = nullptr;
    int64_t c_bstride = 0, c_cstride = 0;
    const float* prev = nullptr;
    int64_t prev_bstride = 0;
    float* out = nullptr;
    int64_t out_bstride = 0;
    int B = 0;
    int T = 0;         // frames the launches cover
    int T_valid = -1;  // (<= T, default T): frames that exist in c / out (bucketed non-AR lengths)
    int f0 = 0;        // the forward covers frames [f0, f0 + T) of every utterance
    const int32_t* seq_len = nullptr;  // utterance b has seq_len[b] frames (device array, null = all equal)
    const int2* slots = nullptr;       // packed AR loop / streaming step: sequence b is (utterance, first frame) slots[b]
    // conditioning inputs / extra output (hificar_forward_cond)
    const int32_t* spk_id = nullptr;
    const int32_t* ph = nullptr;
    int ph_stride = 0;
    float* ph_out = nullptr;
    int ph_out_T = 0;
    // streaming steps (hificar_ar_step): the caller's AR context arena (one row of ar_input samples per session) that replaces prev,
    // the step table {row, frame, valid, first} as the device reads it, and where front_kernel publishes its slots / valid frames
    float* ctx = nullptr;
    const int4* seqs = nullptr;
    int2* seqs_slots = nullptr;
    int* seqs_valid = nullptr;
    const Tape* tp = nullptr;  // training forward: where the activations are kept
    Workspace ws = {};
    hipStream_t stream = nullptr;
};

// Ragged batch context of the launches of one forward: utterance b has seq_len[b] frames (device array, null = all equal); the forward
// covers frames [f0, f0 + frames) of every utterance.
struct Ragged {
    const int32_t* seq_len = nullptr;
    int const_len = -1;  // >= 0 (and seq_len null): every utterance has this many frames, fewer than the launch covers (bucketed lengths)
    int f0 = 0;
    int frames = 0;
    float* ctx = nullptr;  // streaming steps (FwdCall::ctx): the output conv writes out densely by sequence and refreshes the context rows
};

static Ragged ragged_of(const FwdCall& k) {  // (k.T_valid resolved: forward_impl)
    Ragged rg;
    rg.seq_len = k.seq_len;
    rg.const_len = k.T_valid < k.T ? k.f0 + k.T_valid : -1;
    rg.f0 = k.f0;
    rg.frames = k.T;
    rg.ctx = k.ctx;
    return rg;
}

// Launch geometry of a non-AR forward is rounded up to a bucket of frames (the extra frames are masked exactly like the tail of a
// ragged batch: bit-identical results), so that a dataset of many distinct utterance lengths shares launch shapes / schedules.
static int bucket_frames(int T) { return T <= 32 ? T : round_up(T, 32); }

static void fill_params(ConvParams& p, const ConvLayer& L, int rows, int TM, const float* res, float* y, const Ragged& rg) {
    p.seq_len = rg.seq_len;
    p.len_const = rg.seq_len ? -1 : rg.const_len;
    p.len_f0 = rg.f0;
    p.len_max = rg.frames;
    p.len_mul = rg.frames > 0 ? rows / rg.frames : 1;
    p.w16 = reinterpret_cast<const bf16x8*>(L.d_w16);
    p.n_blocks32 = L.n_blocks32;
    p.nb32_per_phase = L.nb32_per_phase;
    p.bias = L.d_bias;
    p.res = res;
    p.y = y;
    p.L = rows;
    p.tiles_per_seq = (rows + TM - 1) / TM;
    p.cin = L.cin_pad;
    p.cout_total = L.cout_total;
    p.ntaps = L.ntaps;
    p.off_min = L.off_min;
    p.halo = L.off_max - L.off_min;
    p.tap_step = L.ntaps > 1 ? L.tap_off[0][1] - L.tap_off[0][0] : 0;
    for (int r = 0; r < kMaxPhase; ++r) p.tap_off0[r] = r < L.n_phase ? L.tap_off[r][0] : 0;
}

static constexpr size_t kArenaBytes = 16u << 20;
static constexpr size_t kMaxArenas = 8;

static int arena_add(hificar_engine* h, size_t min_bytes) {
    hificar_engine::Arena a;
    a.cap = std::max(kArenaBytes, round_up_sz(min_bytes, 4096));
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, a.cap));
    a.d = static_cast<char*>(p);
    hipError_t e = hipHostMalloc(&p, a.cap, hipHostMallocDefault);
    if (e != hipSuccess) {
        (void)hipFree(a.d);
        return fail(HIFICAR_E_HIP, "hipHostMalloc(schedule arena) failed: %s", hipGetErrorString(e));
    }
    a.h = static_cast<char*>(p);
    h->arenas.push_back(a);
    return HIFICAR_OK;
}

// Drops every launch plan together with the schedules they point to, and recycles the arenas: the one place either goes (a very
// large number of distinct launch shapes; rare, off the hot path: hificar_forward buckets non-AR lengths so that shapes repeat).
// Kernels in flight may still read old schedules, so the device is drained first.
static int evict_plans(hificar_engine* h) {
    HIP_TRY(hipDeviceSynchronize());
    h->plans.clear();
    for (auto& a : h->arenas) a.used = 0;
    std::sort(h->arenas.begin(), h->arenas.end(), [](const hificar_engine::Arena& x, const hificar_engine::Arena& y) { return x.cap < y.cap; });
    return HIFICAR_OK;
}

typedef std::vector<std::vector<int>> TileLists;  // an explicit tile list per workgroup, walked in the order given

// Longest-processing-time-first assignment of `costs.size()` tiles to G workgroups; each workgroup's list is then
// ordered light -> heavy (the kernel walks it in that order).
static TileLists lpt_lists(const std::vector<double>& costs, int G) {
    const int n = (int)costs.size();
    std::vector<int> order(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return costs[a] > costs[b]; });
    TileLists lists(G);
    typedef std::pair<double, int> Load;  // (load, workgroup): least loaded first, ties to the lower workgroup
    std::priority_queue<Load, std::vector<Load>, std::greater<Load>> heap;
    for (int w = 0; w < G; ++w) heap.push({0.0, w});
    for (int t : order) {
        Load top = heap.top();
        heap.pop();
        lists[top.second].push_back(t);
        top.first += costs[t];
        heap.push(top);
    }
    for (auto& l : lists) std::reverse(l.begin(), l.end());  // heavy-first insertion order -> light first
    return lists;
}

// One round of tiles of ONE layer whose weights do not fit an XCD's 4-MB L2 (the discriminators' 1024-wide GEMM-form layers: 21 MB of weights,
// 17 row tiles x 8 channel groups): dealt out round-robin every XCD streams ALL the weights through its L2 (335 MB per launch); here every XCD
// gets a BLOCK of (row tiles x channel groups), so that both operands are re-used inside the XCD by workgroups that run in lock step — the
// split of the 8 XCDs into (pr x pg) that minimises row tiles / pr + channel groups / pg.  Workgroup w is dispatched to XCD w % 8
// (MI355X_MICROARCH.md: round-robin; an assumption for speed only — any mapping is correct).
// R row tiles x Gc channel groups, tile id = channel group * R + row tile; XCD x's l-th tile goes to workgroup 8 l + x.  Empty: no split is worth
// it, or the blocks need more than num_cus workgroups.
static TileLists xcd_block_lists(int R, int Gc, int num_cus) {
    int bpr = 1, bpg = 8;
    double bcost = 1e300;
    for (int pr = 1; pr <= 8; pr *= 2) {
        const int pg = 8 / pr;
        if (pr > R || pg > Gc) continue;
        const double c = (double)((R + pr - 1) / pr) + (double)((Gc + pg - 1) / pg);
        if (c < bcost) bcost = c, bpr = pr, bpg = pg;
    }
    const size_t maxblock = (size_t)((R + bpr - 1) / bpr) * ((Gc + bpg - 1) / bpg);
    if (maxblock * 8 > (size_t)num_cus || bcost >= (double)(R + 1)) return TileLists();
    TileLists lists(maxblock * 8);
    for (int x = 0; x < 8; ++x) {
        const int xr = x / bpg, xg = x % bpg;
        size_t l = 0;
        for (int g2 = Gc * xg / bpg; g2 < Gc * (xg + 1) / bpg; ++g2)
            for (int r2 = R * xr / bpr; r2 < R * (xr + 1) / bpr; ++r2) lists[l++ * 8 + (size_t)x].push_back(g2 * R + r2);
    }
    return lists;
}

// The schedule `lists` of n tiles into the arenas (device block + the pinned host mirror it is filled in), uploaded asynchronously on the
// launch stream: the launch that follows is ordered behind the copy, hificar_ar_loop's second stream behind sched_up_seq.
static int upload_schedule(hificar_engine* h, const TileLists& lists, int n, hipStream_t stream, const int** d_start, const int** d_tiles) {
    const int G = (int)lists.size();
    const size_t n_start = round_up_sz((size_t)G + 1, 4);
    const size_t bytes = (n_start + (size_t)std::max(n, 1)) * sizeof(int), take = round_up_sz(bytes, 256);
    if (h->arenas.empty() || h->arenas.back().used + take > h->arenas.back().cap) {
        int rc = h->arenas.size() >= kMaxArenas ? evict_plans(h) : arena_add(h, take);  // (allocates: only when the pre-allocated arena is full)
        if (rc != HIFICAR_OK) return rc;
        if (take > h->arenas.back().cap) return fail(HIFICAR_E_INVALID, "tile schedule of %zu bytes exceeds the arena", take);
    }
    hificar_engine::Arena& a = h->arenas.back();
    int* start = reinterpret_cast<int*>(a.h + a.used);
    int* tiles = start + n_start;
    int pos = 0;
    for (int w = 0; w < G; ++w) {
        start[w] = pos;
        for (int t : lists[w]) tiles[pos++] = t;
    }
    start[G] = pos;
    *d_start = reinterpret_cast<int*>(a.d + a.used);
    *d_tiles = *d_start + n_start;
    a.used += take;
    HIP_TRY(hipMemcpyAsync(const_cast<int*>(*d_start), start, bytes, hipMemcpyHostToDevice, stream));  // pinned source, never rewritten while its plan lives
    ++h->sched_up_seq;
    return HIFICAR_OK;
}

// Order this call's work behind the previous call's when the caller changed streams (shared handle state: schedules, step
// table, workspace).  Same stream: nothing to do.
static int enter_stream(hificar_engine* h, hipStream_t stream) {
    if (h->have_last_stream && h->last_stream != stream) {
        if (h->done_valid && h->done_stream == h->last_stream) {  // the previous call marked its own end: wait for that, not for later work
            HIP_TRY(hipStreamWaitEvent(stream, h->done_ev, 0));
        } else {
            if (!h->xstream_ev) HIP_TRY(hipEventCreateWithFlags(&h->xstream_ev, hipEventDisableTiming));
            HIP_TRY(hipEventRecord(h->xstream_ev, h->last_stream));
            HIP_TRY(hipStreamWaitEvent(stream, h->xstream_ev, 0));
        }
    }
    h->done_valid = false;
    h->last_stream = stream;
    h->have_last_stream = true;
    return HIFICAR_OK;
}

struct TileCfg {
    int MI, WM, WN;
    int KS;  // 1: each MFMA wave owns a 32-channel block of the tile; 4: the four MFMA waves split the K loop of ONE block (WM = WN = 1)
    int NB;  // channel blocks per MFMA wave (conv_ws_body's register blocking, bf16x3 only): tile = WM*MI*32 rows x WN*NB*32 channels
};
static size_t out_buf_bytes(const TileCfg& t) { return (size_t)t.KS * (t.WM * t.MI * 32) * (t.WN * t.NB * 32 + 4) * sizeof(float); }
// preference order: ties keep the earlier entry (taller wave tiles re-read fewer weights per MFMA)
constexpr int kNumTileCfgs = 15;
static const TileCfg kTileCfgs[kNumTileCfgs] = {{4, 1, 4, 1, 1}, {4, 2, 2, 1, 1}, {4, 4, 1, 1, 1}, {2, 2, 2, 1, 2}, {2, 4, 1, 1, 2},
                                                {2, 1, 4, 1, 2}, {2, 1, 4, 1, 1}, {2, 2, 2, 1, 1}, {2, 4, 1, 1, 1},
                                                {1, 1, 4, 1, 1}, {1, 2, 2, 1, 1}, {1, 4, 1, 1, 1}, {4, 1, 1, 4, 1}, {2, 1, 1, 4, 1}, {1, 1, 1, 4, 1}};

// One conv launch on activated rows (either arithmetic).  Per branch: xs (activated input) -> y (fp32, nullable) and/or ys (split copy of
// LeakyReLU(out, slope_out), nullable), + optional fp32 residual.
struct ConvIO {
    const char* xs;
    const float* res;
    float* y;
    char* ys;
    const float* mask_src = nullptr;  // backward launches: LeakyReLU'(mask_src) scales the result before res is added
    float mask_slope = 0.f;
    long long x_seq_bytes = 0;        // input row addressing (ConvParams::x_seq_bytes / x_row_bytes); 0: packed rows
    int x_row_bytes = 0;
    int x_rows = 0;                   // input rows per sequence when they differ from the launch's rows (ConvParams::x_rows)
    int x_up = 0;                     // nearest-neighbour upsampling of the input rows while staging (ConvParams::x_up); the input then has rows / x_up rows
    float x_slope = -1.f;             // >= 0: xs holds PRE-activation fp32 rows, LeakyReLU(x_slope) is applied while staging (ConvParams::act_in; exact fp32 only)
    const float* x_more[3] = {nullptr, nullptr, nullptr};  // ... and the input is the mean of xs and these further streams (x_n in all), summed in this order
    int x_n = 1;
    bool res_relu = false;            // res holds the rows before their ReLU (ConvParams::res_relu; bf16x3 dense launches only)
};

// Replicas of every branch at regular strides (the groups of a grouped conv): see MultiConvParams::zrep
struct ConvRep {
    int n = 1;
    long long zs_x = 0, zs_w = 0, zs_y = 0, zs_b = 0;
};

// Whether a launch of these branches can run tile shape t at all: the instantiations that exist, the LDS budget, and what the register-blocked
// and split-K forms need of the layers.  halo_all: the widest branch's off_max - off_min; nsteps_min: the shortest branch's (tap, slab) steps
// per K chunk.  Shared by the cost loop of pick_tile and by a forced shape (hificar_debug_force_tile).
static bool tile_admissible(const hificar_engine* h, const ConvLayer* const* layers, int nbr, const TileCfg& t, int halo_all, int nsteps_min) {
    const ConvLayer& L0 = *layers[0];
    const bool f32 = h->precision == HIFICAR_PREC_F32;
    const int TM = t.WM * t.MI * 32, RB = L0.chunk16 * 4;
    if (t.NB == 2 && (f32 || L0.chunk16 == 16)) return false;  // (not instantiated)
    const size_t obuf = (f32 && t.KS == 1) ? 0 : out_buf_bytes(t);
    if (2 * round_up_sz((size_t)(TM + halo_all) * RB, 1024) + obuf > 160 * 1024) return false;
    if (t.NB == 2) {  // a wave's two channel blocks share the activation fragments: same phase of a polyphase (transposed) conv
        bool ok = L0.n_blocks32 >= 2;
        for (int b = 0; b < nbr; ++b) ok = ok && (layers[b]->n_phase == 1 || layers[b]->nb32_per_phase % 2 == 0);
        if (!ok) return false;
    }
    if (t.KS == 4 && (h->ksplit == 0 || nsteps_min < 2)) return false;
    return true;
}

// Tile shape of a launch_conv launch: simulate the kernel's tile walk and take the shape with the smallest makespan.  A tile costs its
// MFMA issue cycles (all four MFMA waves run in lock step: 3*MI MFMAs of 32 cycles per 16-channel K slab) plus a fixed per-tile and
// per-item overhead.  Pure host arithmetic on the launch shape and the engine's fixed switches.
// merged: the branch-summing launch (conv_f32mrg_kernel) — a tile is a POSITION, whose workgroup runs the K loops of all nbr branches one after the
// other and one epilogue: dense one-block shapes only.  est: the chosen shape's estimated makespan in cycles (1e300: no shape can run).
// use_force = false: the planner's own choice even while a test forces a shape (build_merge_plan's estimates: which FORM runs must not depend on the hook).
static TileCfg pick_tile(const hificar_engine* h, const ConvLayer* const* layers, int nbr, int nseq, int rows, int zrep, bool merged = false,
                         double* est = nullptr, bool use_force = true) {
    const ConvLayer& L0 = *layers[0];
    const bool f32 = h->precision == HIFICAR_PREC_F32;  // rows are plain fp32 LeakyReLU(x) instead of split rows
    int halo_all = 0;
    for (int b = 0; b < nbr; ++b) halo_all = std::max(halo_all, layers[b]->off_max - layers[b]->off_min);
    TileCfg tc = {1, 4, 1, 1, 1};
    double best = 1e300;
    // The dense exact-fp32 launches are direct-output (conv_f32do_kernel): tiles stored straight from the MFMA waves' accumulators, no LDS out-buffer
    // (its bytes are free for taller tiles / wider halos below).  The register-blocked (NB = 2) wave tiles exist in bf16x3 only, where the cost model
    // may prefer them (+1.3 %; in exact fp32 they measured -1.0 %: profiles/r04_nb_register_blocking.txt).
    int nsteps_min = 1 << 30;
    for (int b = 0; b < nbr; ++b) nsteps_min = std::min(nsteps_min, layers[b]->ntaps * (L0.chunk16 / 16));
    if (h->force_tile[0] != 0 && use_force) {  // a test's forced shape (hificar_debug_force_tile), where this launch can run it; otherwise the normal choice below
        const TileCfg t = {h->force_tile[0], h->force_tile[1], h->force_tile[2], h->force_tile[3], h->force_tile[4]};
        if (tile_admissible(h, layers, nbr, t, halo_all, nsteps_min) && (!merged || (t.KS == 1 && t.NB == 1))) return t;
    }
    for (int ti = 0; ti < kNumTileCfgs; ++ti) {
        const TileCfg& t = kTileCfgs[ti];
        const int TM = t.WM * t.MI * 32;
        const int chunk = L0.chunk16;
        if (!tile_admissible(h, layers, nbr, t, halo_all, nsteps_min)) continue;
        if (merged && (t.KS != 1 || t.NB != 1)) continue;
        if (!merged && t.KS == 1 && h->ksplit == 2 && nsteps_min >= 2) continue;
        const long long tiles_per_branch = (long long)nseq * ((rows + TM - 1) / TM) * ((L0.n_blocks32 + t.WN * t.NB - 1) / (t.WN * t.NB));
        const int ncls = merged ? 1 : nbr;  // cost classes of tiles: the branches, or (merged) the one kind of position
        const long long total = tiles_per_branch * ncls * zrep;
        const int G = (int)std::min<long long>(total, h->num_cus);
        const int nchunks = L0.cin_pad / chunk;
        // LPT makespan estimate: max(heaviest tile, total / G), plus one light tile when the count does not divide
        double total_cost = 0.0, heaviest = 0.0, lightest = 1e300, cb[3] = {0.0, 0.0, 0.0};
        for (int b = 0; b < nbr; ++b) {
            // MFMA issue cycles per 16-channel slab and 32x32 accumulator: 3 x 32 (bf16x3, ~75 % sustained) or 8 x 64 (fp32)
            const double slab = f32 ? 8 * 64.0 : 3 * 32 / 0.75;
            double c = (double)layers[b]->ntaps * (L0.cin_pad / 16) * slab * t.MI * t.NB + 2500.0 + 400.0 * nchunks;
            if (t.KS == 4) {
                // each wave runs ceil(steps / 4) of an item's (tap, slab) steps; exposed weight latency at every tile start, the partial
                // sums' extra pass, and four times the staging per output
                const int steps = layers[b]->ntaps * (chunk / 16);
                c = (double)((steps + 3) / 4) * nchunks * slab * t.MI + 4000.0 + 600.0 * nchunks;
            }
            if (merged) {  // one position: every branch's K loop, one tile set-up and epilogue, every branch's items
                cb[0] += c - (b ? 2500.0 : 0.0);
                continue;
            }
            total_cost += c * tiles_per_branch * zrep;
            heaviest = std::max(heaviest, c);
            lightest = std::min(lightest, c);
            cb[b] = c;
        }
        if (merged) {
            total_cost = cb[0] * tiles_per_branch * zrep;
            heaviest = lightest = cb[0];
        }
        double worst = std::max(heaviest, total_cost / G);
        if (!h->shared_chip && total > G && total <= 4096) {
            // the makespan of the assignment the kernel will actually walk (lpt_lists: longest tile first onto the least loaded workgroup).
            // Round 4: the closed form below charged "+ half a light tile" whenever the tile count is not a multiple of the workgroups — 384
            // tiles of weight 12 : 8 : 4 on 256 workgroups balance exactly (12 | 8 + 4), and the 128-row tile it ruled out at C = 256 is 1.1 %
            // faster end to end than the 64-row one it picked.
            std::sort(cb, cb + ncls, [](double x, double y) { return x > y; });
            std::priority_queue<double, std::vector<double>, std::greater<double>> load;
            for (int w = 0; w < G; ++w) load.push(0.0);
            worst = 0.0;
            for (int b = 0; b < ncls; ++b)
                for (long long i = 0; i < tiles_per_branch * zrep; ++i) {
                    const double v = load.top() + cb[b];
                    load.pop();
                    load.push(v);
                    worst = std::max(worst, v);
                }
        } else if (total % G != 0) {
            worst = std::max(worst, total_cost / G + 0.5 * lightest);
        }
        // An engine whose launches overlap with others on side streams (the discriminators): a launch's own makespan — a nearly empty
        // last round, a chip half filled by tall tiles — is filled by the neighbours' workgroups, so what counts is the workgroup-time the
        // shape costs, i.e. its efficiency per tile.  (Measured: discriminator step 20.6 -> 19.9 ms, generator-side pass 10.7 -> 10.0 ms;
        // launches with fewer tiles than pick_throughput stay latency-driven.)
        if (h->pick_throughput > 0 && total >= h->pick_throughput) worst = total_cost / h->num_cus;
        // shorter wave tiles re-read the weight stream more often per MFMA (MI = 2 measured ~10 % slower per flop)
        // operand loads per MFMA: 2 (MI + NB) 16-byte loads per slab step against (8 | 3) MI NB MFMAs
        if (t.NB == 2) worst *= f32 ? (t.MI == 4 ? 0.95 : t.MI == 2 ? 0.975 : 1.02) : (t.MI == 2 ? 0.93 : 1.10);
        else if (t.MI < 4) worst *= f32 ? (t.MI == 2 ? 1.02 : h->mi1_penalty) : (t.MI == 2 ? 1.10 : 1.25);
        if (t.KS == 4) worst *= 1.05;  // near-ties go to the dense form
        if (worst < best * 0.98) {  // near-ties keep the earlier (taller) shape
            best = worst;
            tc = t;
        }
    }
    if (est) *est = best;
    return tc;
}

// Kernel name of a plan as ProfScope wants it: the instantiation (hificar_launch.h), + "|layer xN" for per-layer rows in the profile (tools/layer_profile.py);
// "|layer +N": the N branches summed in one accumulator (launch_merged) instead of side by side
static std::string plan_name(const hificar_engine* h, const ConvShape& s, const ConvLayer& L0, int nbr) {
    static const char* const family[] = {"conv_f32do_kernel", "conv_bf16x3_kernel", "conv_bf16x3nb_kernel", "conv_sk_f32_kernel", "conv_sk_bf16x3_kernel",
                                         "conv_pair_f32_kernel", "conv_pair_bf16x3_kernel", "conv_f32mrg_kernel"};
    char kname[96];
    int n = s.family == kConvSkF32 || s.family == kConvSkBf16x3 ? snprintf(kname, sizeof(kname), "%s<%d,%d>", family[s.family], s.mi, s.nc16)
                                                                : snprintf(kname, sizeof(kname), "%s<%d,%d,%d,%d>", family[s.family], s.mi, s.wm, s.wn, s.nc16);
    if (h->profile_detail) snprintf(kname + n, sizeof(kname) - n, s.family == kConvF32mrg ? "|%s +%d" : "|%s x%d", L0.name.c_str(), nbr);
    return kname;
}

static int build_conv_plan(hificar_engine* h, const ConvLayer* const* layers, int nbr, int nseq, int rows, int zrep, hipStream_t stream, ConvPlan& pl) {
    const ConvLayer& L0 = *layers[0];
    const bool f32 = h->precision == HIFICAR_PREC_F32;
    MultiConvParams& mp = pl.conv;
    const TileCfg tc = pick_tile(h, layers, nbr, nseq, rows, zrep);
    int halo_all = 0;
    for (int b = 0; b < nbr; ++b) halo_all = std::max(halo_all, layers[b]->off_max - layers[b]->off_min);
    const int TM = tc.WM * tc.MI * 32, nc16 = L0.chunk16 / 16;
    const size_t buf_bytes = round_up_sz((size_t)(TM + halo_all) * L0.chunk16 * 4, 1024);
    const bool dout = f32 && tc.KS == 1;
    pl.shape = {dout ? kConvF32do : tc.KS == 4 ? (f32 ? kConvSkF32 : kConvSkBf16x3) : tc.NB == 2 ? kConvBf16x3nb : kConvBf16x3, tc.MI, tc.WM, tc.WN, nc16};
    pl.lds = 2 * buf_bytes + (dout ? 0 : out_buf_bytes(tc));
    mp.buf_bytes = (int)buf_bytes;
    mp.n_branches = nbr;
    mp.nseq_tiles = nseq * ((rows + TM - 1) / TM);
    mp.ngroups = (L0.n_blocks32 + tc.WN * tc.NB - 1) / (tc.WN * tc.NB);
    mp.total_tiles = nbr * zrep * mp.ngroups * mp.nseq_tiles;
    pl.grid = (unsigned)std::min(mp.total_tiles, h->num_cus);  // persistent: one workgroup per CU walks its tile list
    {   // one round of tiles and at least twice the activations in weight bytes (batch 8 measured neutral at 1.8 x): XCD-contiguous tile order (MultiConvParams::xcd_order)
        double wbytes = 0.0;
        for (int b = 0; b < nbr; ++b) wbytes += 4.0 * layers[b]->cin_pad * layers[b]->cout_total * layers[b]->ntaps * zrep;
        const double abytes = 4.0 * nseq * rows * L0.cin_pad * nbr * zrep;
        mp.xcd_order = (mp.total_tiles <= h->num_cus && mp.total_tiles >= 16 && wbytes > 2.0 * abytes) ? 1 : 0;
    }
    // every input row is staged once per channel group: more than two groups (upsampler 0's ten, a 1024-wide GEMM's eight) re-read it from the L2
    // instead of streaming it past the cache (r06a: 2.7 x / 3-7 x the algorithmic bytes fetched by those launches with non-temporal loads)
    mp.stage_cached = mp.ngroups > 2 ? 1 : 0;
    pl.name = plan_name(h, pl.shape, L0, nbr);
    TileLists lists;
    if (mp.total_tiles <= h->num_cus && nbr == 1 && zrep == 1 && mp.ngroups >= 2 && mp.nseq_tiles >= 8 && !h->shared_chip &&
        4.0 * L0.cin_pad * L0.cout_total * L0.ntaps > 6.0e6)  // (one layer's weights well beyond an XCD's L2)
        lists = xcd_block_lists(mp.nseq_tiles, mp.ngroups, h->num_cus);
    if (!lists.empty()) {
        pl.grid = (unsigned)lists.size();
        mp.xcd_order = 0;
    } else if (mp.total_tiles > (int)pl.grid) {
        std::vector<double> costs((size_t)mp.total_tiles);
        const int tpb = mp.ngroups * mp.nseq_tiles * zrep;
        for (int b = 0; b < nbr; ++b)
            for (int i = 0; i < tpb; ++i) costs[(size_t)b * tpb + i] = layers[b]->ntaps + 1.0;  // + fixed per-tile overhead
        lists = lpt_lists(costs, (int)pl.grid);
    }
    return lists.empty() ? HIFICAR_OK : upload_schedule(h, lists, mp.total_tiles, stream, &mp.sched_start, &mp.sched_tiles);
}

// The branch-summing launch (conv_f32mrg_kernel): the last ResBlock layers of ALL nbr blocks of a stage, whose workgroups run the K loops of the nbr
// branches of a position — (sequence, row tile, channel group) — into the same accumulators and write the activated MRF mean once.  Tiles are
// positions: ngroups x nseq_tiles of them, each costing the sum of its branches' taps + 1, all alike — position q goes to workgroup q mod G, and a
// workgroup's list holds, per position, the nbr tile ids (branch-major, as conv_ws_body decodes them) in launch order: always an explicit list.
// merge_wins: this launch is estimated to beat the side-by-side launches of the same layers (groups
// of up to three, launch_n) by more than the folded mean costs the upsampler — its loader waves re-read (nbr - 1) further fp32 streams, at best
// at the HBM's ~2 KB per cycle (the measured difference, profiles/r06a vs r06 by layer, is 1.5 x that) — so small launches stay side by side.
static int build_merge_plan(hificar_engine* h, const ConvLayer* const* layers, int nbr, int nseq, int rows, hipStream_t stream, ConvPlan& pl) {
    const ConvLayer& L0 = *layers[0];
    MergeConvParams& mp = pl.merge;
    double est_merged = 1e300, est_classic = 0.0;
    const TileCfg tc_free = pick_tile(h, layers, nbr, nseq, rows, 1, true, &est_merged, false);
    const TileCfg tc = pick_tile(h, layers, nbr, nseq, rows, 1, true);  // (a forced shape where the launch can run it)
    if (est_merged >= 1e300) return fail(HIFICAR_E_INVALID, "internal: no tile shape for the merged launch of %s", L0.name.c_str());
    for (int q0 = 0; q0 < nbr; q0 += 3) {
        double e = 0.0;
        (void)pick_tile(h, layers + q0, std::min(3, nbr - q0), nseq, rows, 1, false, &e, false);
        est_classic += e;
    }
    const double up_extra = 4.0 * nseq * rows * L0.cout_total * (nbr - 1) / 2048.0;
    // Two cases the estimate does not cover stay side by side (measured, profiles/r07_batch_sizes.txt): the halves of a batch on two streams (shared_chip:
    // pick_tile does not simulate the walk there, and a third of the tiles leaves the other half's launches less to overlap with: batch 32 -2 %),
    // and a merged launch that would need 32-row wave tiles to spread (MI = 1 re-streams the weights most often and a position's K loop is n times
    // as long: batch 16 -0.15 %)
    pl.merge_wins = !h->shared_chip && tc_free.MI > 1 && est_merged < est_classic + up_extra;
    if (!pl.merge_wins && h->mrf_merge != 2) return HIFICAR_OK;  // (the plan only records the decision: no schedule for a launch that will not run)
    int halo_all = 0;
    for (int b = 0; b < nbr; ++b) halo_all = std::max(halo_all, layers[b]->off_max - layers[b]->off_min);
    const int TM = tc.WM * tc.MI * 32, nc16 = L0.chunk16 / 16;
    const size_t buf_bytes = round_up_sz((size_t)(TM + halo_all) * L0.chunk16 * 4, 1024);
    pl.shape = {kConvF32mrg, tc.MI, tc.WM, tc.WN, nc16};
    pl.lds = 2 * buf_bytes;
    mp.buf_bytes = (int)buf_bytes;
    mp.n_branches = nbr;
    mp.nseq_tiles = nseq * ((rows + TM - 1) / TM);
    mp.ngroups = (L0.n_blocks32 + tc.WN - 1) / tc.WN;
    const int npos = mp.ngroups * mp.nseq_tiles;
    mp.total_tiles = nbr * npos;
    pl.grid = (unsigned)std::min(npos, h->num_cus);
    mp.xcd_order = 0;
    mp.stage_cached = mp.ngroups > 2 ? 1 : 0;
    pl.name = plan_name(h, pl.shape, L0, nbr);
    TileLists lists(pl.grid);
    for (int q = 0; q < npos; ++q)
        for (int b = 0; b < nbr; ++b) lists[(size_t)q % pl.grid].push_back(b * npos + q);
    return upload_schedule(h, lists, mp.total_tiles, stream, &mp.sched_start, &mp.sched_tiles);
}

// Fused conv1 -> LeakyReLU -> conv2 (+ residual) for C = 32 / 64 (conv_pair_bf16x3_kernel / conv_pair_f32_kernel).
struct PairIOB {
    const float* xf;  // fp32 pre-activation input of conv1 (activated + split while staging), or null when xs is given
    const char* xs;   // split input of conv1
    const float* res; // fp32 residual
    float* y;         // fp32 output (may alias res)
    char* ys;         // split copy of LeakyReLU(y) for the next pair (must NOT alias xs: neighbouring tiles read xs halos), or null
};

// Launches with too few 512-row tiles to fill the chip at C = 32 in exact fp32 (batch 8 with chunks of 25 frames): 128-row tiles (MI = 1)
// — a tile's serial MFMA chain is a quarter as long and four times as many workgroups have work, so the fused pair beats two dependent
// launches there (measured batch 8: +2.7 % end to end).  Below ~8000 rows (batch 1: 2000) the split-K layer-by-layer launches, whose chains
// are shorter still, stay ahead (measured batch 1: -3.6 % with the fused form), so those keep running layer by layer.
static bool pair_small_tiles(const hificar_engine* h, int C, int k2, int nseq, int rows) {
    // (HIFICAR_KSPLIT=0, the batch-invariant mode: no launch-size-dependent forms at small sizes)
    if (!h->pair_small || h->ksplit == 0 || C != 32 || h->precision != HIFICAR_PREC_F32 || nseq <= 0 || (long long)nseq * rows < 8000) return false;
    const int tmo = 4 * 4 * 32 - (k2 - 1);
    return 3LL * nseq * ((rows + tmo - 1) / tmo) < h->num_cus;
}

// nseq / rows: the launch the pair would run in (0 / 0: only the static conditions)
static bool pair_eligible(const hificar_engine* h, const ConvLayer& a, const ConvLayer& b, int nseq = 0, int rows = 0) {
    if (!(h->use_pair && a.d_w16c && b.d_w16c && a.d_w32c && b.d_w32c && a.cin == b.cin && a.ntaps >= 2 &&
          b.ntaps >= 2 && b.dilation == 1 && a.K == b.K))
        return false;
    // the LDS budget of launch_pair (wide dilations x long kernels do not fit: those pairs run layer by layer)
    const int C = a.cin, TMc = (C == 64 ? 2 : 4) * 4 * 32;
    const size_t in_bytes = round_up_sz((size_t)(TMc + a.off_max - a.off_min) * C * 4, 1024);
    const size_t ts_bytes = std::max<size_t>((size_t)(TMc + 16) * C * 4, (size_t)TMc * (C + 4) * sizeof(float));
    if (in_bytes + ts_bytes > 160 * 1024) return false;
    if (nseq > 0) {
        // The fused kernel's tiles are tall (TMc conv1 rows for TMc - (k-1) output rows).  (i) A launch with few tiles leaves most
        // CUs idle behind long serial tiles: small batches run layer by layer.  (ii) Tile quantisation: 1000 rows at k = 11 need 5
        // tiles of 256 (28 % extra conv1 work); the exact-fp32 arithmetic gains little from fusion (its layer-by-layer kernels are
        // matrix-pipe-bound already), so it only fuses when the waste is small; the bf16x3 ones are memory-path-bound and gain more.
        if (pair_small_tiles(h, C, b.ntaps, nseq, rows)) return true;
        const int tmo = TMc - (b.ntaps - 1);
        const long long tiles = (long long)nseq * ((rows + tmo - 1) / tmo);
        if (3 * tiles < h->num_cus) return false;
        const double waste = (double)((rows + tmo - 1) / tmo) * TMc / rows;
        if (waste > (h->precision == HIFICAR_PREC_F32 ? 1.12 : 1.35)) return false;
    }
    return true;
}

static int build_pair_plan(hificar_engine* h, const ConvLayer* const* l1, const ConvLayer* const* l2, int nbr, int nseq, int rows, hipStream_t stream,
                           ConvPlan& pl) {
    const int C = l1[0]->cin;
    bool small = true;
    for (int b = 0; b < nbr; ++b) small = small && pair_small_tiles(h, C, l2[b]->ntaps, nseq, rows);
    const int MI = small ? 1 : 4, WM = C == 64 ? 2 : 4;
    const int TMc = WM * MI * 32, RB = C * 4;
    const bool f32 = h->precision == HIFICAR_PREC_F32;
    PairParams& pp = pl.pair;
    int halo_max = 0, tile = 0;
    for (int b = 0; b < nbr; ++b) {
        halo_max = std::max(halo_max, l1[b]->off_max - l1[b]->off_min);
        const int tmo = TMc - (l2[b]->ntaps - 1);
        pp.tiles_per_seq[b] = (rows + tmo - 1) / tmo;
        pp.tile_start[b] = tile;
        tile += nseq * pp.tiles_per_seq[b];
    }
    pp.tile_start[nbr] = tile;
    pp.n_branches = nbr;
    pp.nseq = nseq;
    pp.in_bytes = (int)round_up_sz((size_t)(TMc + halo_max) * RB, 1024);
    pp.ts_bytes = (int)std::max<size_t>((size_t)(TMc + 16) * RB, (size_t)TMc * (C + 4) * sizeof(float));  // TS and out-buffer alias
    pl.lds = (size_t)pp.in_bytes + pp.ts_bytes;
    if (pl.lds > 160 * 1024) return fail(HIFICAR_E_INVALID, "internal: pair kernel LDS too large (%zu)", pl.lds);
    pl.grid = (unsigned)std::min(tile, h->num_cus);
    pl.shape = {f32 ? kPairF32 : kPairBf16x3, MI, WM, 4 / WM, C / 16};
    pl.name = plan_name(h, pl.shape, *l1[0], nbr);
    if (tile <= (int)pl.grid) return HIFICAR_OK;
    std::vector<double> costs((size_t)tile);
    for (int b = 0; b < nbr; ++b)
        for (int i = pp.tile_start[b]; i < pp.tile_start[b + 1]; ++i) costs[i] = l1[b]->ntaps + l2[b]->ntaps + 2.0;
    return upload_schedule(h, lpt_lists(costs, (int)pl.grid), tile, stream, &pp.sched_start, &pp.sched_tiles);
}

// The plan of a launch of layers `a` (launch_pair: conv1 `a`, conv2 `b` of every branch), built on the first launch of that shape — only that
// touches vectors, strings or the arenas — on the launch's stream: a new schedule is uploaded on the stream that first needs it (publish()
// in hificar_ar_loop).  Null: failed, *rc says how.
static const ConvPlan* get_plan(hificar_engine* h, const ConvLayer* const* a, const ConvLayer* const* b, int nbr, int nseq, int rows, int zrep,
                                hipStream_t stream, int* rc, bool merged = false) {
    *rc = HIFICAR_OK;
    PlanKey k = {{}, nseq, rows, zrep, (h->precision == HIFICAR_PREC_F32 ? 1 : 0) | (h->training ? 2 : 0) | (h->shared_chip ? 4 : 0) | (b ? 8 : 0) | (merged ? 16 : 0)};
    for (int i = 0; i < nbr; ++i) k.layers[i] = a[i];
    for (int i = 0; b && i < nbr; ++i) k.layers[3 + i] = b[i];
    auto it = h->plans.find(k);
    if (it == h->plans.end()) {
        ConvPlan pl;
        if (h->plans.size() > 20000) *rc = evict_plans(h);  // (a very large number of distinct launch shapes: start over)
        if (*rc == HIFICAR_OK)
            *rc = merged ? build_merge_plan(h, a, nbr, nseq, rows, stream, pl)
                  : b    ? build_pair_plan(h, a, b, nbr, nseq, rows, stream, pl)
                         : build_conv_plan(h, a, nbr, nseq, rows, zrep, stream, pl);
        if (*rc != HIFICAR_OK) return nullptr;
        it = h->plans.emplace(k, std::move(pl)).first;
    }
    return &it->second;
}

static int launch_conv(hificar_engine* h, const ConvLayer* const* layers, int nbr, int nseq, int rows, const ConvIO* io,
                              float slope_out, const Ragged& rg, hipStream_t stream, const ConvRep& zr = ConvRep()) {
    int rc;
    const ConvPlan* const pl = get_plan(h, layers, nullptr, nbr, nseq, rows, zr.n, stream, &rc);
    if (!pl) return rc;
    const int TM = pl->shape.wm * pl->shape.mi * 32;
    const ConvLayer& L0 = *layers[0];
    const bool f32 = h->precision == HIFICAR_PREC_F32;  // rows are plain fp32 LeakyReLU(x) instead of split rows
    MultiConvParams mp = pl->conv;
    double flops = 0.0, bytes = 0.0;
    for (int b = 0; b < nbr; ++b) {
        const ConvLayer& Lb = *layers[b];
        if (Lb.n_blocks32 != L0.n_blocks32 || Lb.chunk16 != L0.chunk16 || Lb.cin_pad != L0.cin_pad)
            return fail(HIFICAR_E_INVALID, "internal: branch shape mismatch");
        fill_params(mp.p[b], Lb, rows, TM, io[b].res, io[b].y, rg);
        mp.p[b].xs = io[b].xs;
        mp.p[b].ys = io[b].ys;
        if (io[b].x_slope >= 0.f) {
            if (!f32) return fail(HIFICAR_E_INVALID, "internal: pre-activation input rows of %s outside the exact-fp32 layer-by-layer launches", Lb.name.c_str());
            if (io[b].x_n < 1 || io[b].x_n > 4) return fail(HIFICAR_E_INVALID, "internal: %d input streams of %s", io[b].x_n, Lb.name.c_str());
            mp.p[b].act_in = io[b].x_n;
            for (int q = 0; q + 1 < io[b].x_n; ++q) mp.p[b].xs_more[q] = reinterpret_cast<const char*>(io[b].x_more[q]);
            mp.p[b].slope_in = io[b].x_slope;
        }
        if (io[b].res_relu) {
            if (f32 || pl->shape.family == kConvSkBf16x3)
                return fail(HIFICAR_E_INVALID, "internal: pre-activation residual rows of %s outside the dense bf16x3 launches", Lb.name.c_str());
            mp.p[b].res_relu = 1;
        }
        mp.p[b].mask_src = io[b].mask_src;
        mp.p[b].mask_slope = io[b].mask_slope;
        mp.p[b].x_seq_bytes = io[b].x_seq_bytes;
        mp.p[b].x_row_bytes = io[b].x_row_bytes;
        mp.p[b].x_rows = io[b].x_rows;
        if (io[b].x_up > 1) {
            if (rows % io[b].x_up != 0 || io[b].x_seq_bytes != 0 || io[b].x_row_bytes != 0)
                return fail(HIFICAR_E_INVALID, "internal: upsampled input rows of %s", Lb.name.c_str());
            mp.p[b].x_up = io[b].x_up;
            mp.p[b].x_up_rcp = (unsigned)(0x100000000ull / (unsigned)io[b].x_up) + 1u;
            mp.p[b].x_seq_bytes = (long long)(rows / io[b].x_up) * Lb.cin_pad * 4;
        }
        mp.p[b].zeros = h->d_zeros;
        mp.p[b].slope_out = slope_out;
        mp.p[b].cout_real = Lb.cout_pad;
        if (f32) mp.p[b].w16 = reinterpret_cast<const bf16x8*>(Lb.d_w32);
        const double pos = (double)nseq * rows;
        flops += 2.0 * pos * Lb.cin * Lb.cout * Lb.K * zr.n;
        bytes += 4.0 * (pos * Lb.cin_pad * (io[b].x_slope >= 0.f ? io[b].x_n : 1) / std::max(1, io[b].x_up) + pos * Lb.cout_total * ((io[b].res ? 1 : 0) + (io[b].y ? 1 : 0) + (io[b].ys ? 1 : 0)) +
                        (double)Lb.cin * Lb.cout * Lb.K);
    }
    mp.zrep = zr.n;
    mp.zs_x = zr.zs_x;
    mp.zs_w = zr.zs_w;
    mp.zs_y = zr.zs_y;
    mp.zs_b = zr.zs_b;
    ProfScope prof(h, stream, pl->name, flops, bytes);
    const hipError_t e = conv_launch(pl->shape, &mp, dim3(pl->grid, 1, 1), pl->lds, stream);
    if (e != hipSuccess) return fail(HIFICAR_E_HIP, "conv launch (%s, %s) failed: %s", L0.name.c_str(), pl->name.c_str(), hipGetErrorString(e));
    return HIFICAR_OK;
}

// The branch-summing launch of layers[0 .. nbr) (2 to 4 blocks): branch b reads the activated rows io[b].xs and adds the residual io[b].res; the one
// output, LeakyReLU(mean of the blocks' outputs, slope_out), goes to ys_out — a buffer no branch reads.  No block's own output is written.
static int launch_merged(hificar_engine* h, const ConvPlan* pl, const ConvLayer* const* layers, int nbr, int nseq, int rows, const ConvIO* io, char* ys_out,
                         float slope_out, const Ragged& rg, hipStream_t stream) {
    const int TM = pl->shape.wm * pl->shape.mi * 32;
    const ConvLayer& L0 = *layers[0];
    MergeConvParams mp = pl->merge;
    double flops = 0.0, bytes = 0.0;
    const double pos = (double)nseq * rows;
    for (int b = 0; b < nbr; ++b) {
        const ConvLayer& Lb = *layers[b];
        if (Lb.n_blocks32 != L0.n_blocks32 || Lb.chunk16 != L0.chunk16 || Lb.cin_pad != L0.cin_pad || Lb.cout_total != L0.cout_total || Lb.n_phase != 1 ||
            !io[b].res || !io[b].xs || io[b].xs == ys_out)
            return fail(HIFICAR_E_INVALID, "internal: merged launch of %s: branch %d does not fit", L0.name.c_str(), b);
        fill_params(mp.p[b], Lb, rows, TM, io[b].res, nullptr, rg);
        mp.p[b].xs = io[b].xs;
        mp.p[b].ys = ys_out;
        mp.p[b].zeros = h->d_zeros;
        mp.p[b].slope_out = slope_out;
        mp.p[b].cout_real = Lb.cout_pad;
        mp.p[b].w16 = reinterpret_cast<const bf16x8*>(Lb.d_w32);
        flops += 2.0 * pos * Lb.cin * Lb.cout * Lb.K;
        bytes += 4.0 * (pos * Lb.cin_pad + pos * Lb.cout_total + (double)Lb.cin * Lb.cout * Lb.K);  // input, residual, weights
    }
    bytes += 4.0 * pos * L0.cout_total;  // the one output
    mp.zrep = 1;
    ProfScope prof(h, stream, pl->name, flops, bytes);
    const hipError_t e = conv_launch(pl->shape, &mp, dim3(pl->grid, 1, 1), pl->lds, stream);
    if (e != hipSuccess) return fail(HIFICAR_E_HIP, "merged conv launch (%s, %s) failed: %s", L0.name.c_str(), pl->name.c_str(), hipGetErrorString(e));
    return HIFICAR_OK;
}

static int launch_pair(hificar_engine* h, const ConvLayer* const* l1, const ConvLayer* const* l2, int nbr, int nseq, int rows,
                              const PairIOB* io, float slope, const Ragged& rg, hipStream_t stream) {
    int rc;
    const ConvPlan* const pl = get_plan(h, l1, l2, nbr, nseq, rows, 1, stream, &rc);
    if (!pl) return rc;
    const int TMc = pl->shape.wm * pl->shape.mi * 32;
    const int C = l1[0]->cin;
    const bool f32 = h->precision == HIFICAR_PREC_F32;
    PairParams pp = pl->pair;
    double flops = 0.0, bytes = 0.0;
    for (int b = 0; b < nbr; ++b) {
        const ConvLayer& A = *l1[b];
        const ConvLayer& B = *l2[b];
        fill_params(pp.p1[b], A, rows, TMc, nullptr, nullptr, rg);
        fill_params(pp.p2[b], B, rows, TMc, io[b].res, io[b].y, rg);
        pp.p1[b].w16 = f32 ? reinterpret_cast<const bf16x8*>(A.d_w32c) : reinterpret_cast<const bf16x8*>(A.d_w16c);
        pp.p2[b].w16 = f32 ? reinterpret_cast<const bf16x8*>(B.d_w32c) : reinterpret_cast<const bf16x8*>(B.d_w16c);
        pp.p1[b].xs = io[b].xs;
        pp.p1[b].xf = io[b].xf;
        pp.p1[b].slope_in = slope;
        pp.p1[b].zeros = h->d_zeros;
        pp.p2[b].ys = io[b].ys;
        pp.p2[b].slope_out = slope;
        pp.p2[b].cout_real = C;
        const double pos = (double)nseq * rows;
        flops += 2.0 * pos * C * C * (A.K + B.K);
        bytes += 4.0 * (pos * C * (3 + (io[b].ys ? 1 : 0)) + (double)C * C * (A.K + B.K));
    }
    pp.slope_mid = slope;
    ProfScope prof(h, stream, pl->name, flops, bytes);
    const hipError_t e = conv_launch(pl->shape, &pp, dim3(pl->grid, 1, 1), pl->lds, stream);
    if (e != hipSuccess) return fail(HIFICAR_E_HIP, "pair launch (%s) failed: %s", l1[0]->name.c_str(), hipGetErrorString(e));
    return HIFICAR_OK;
}

// ------------------------------------------------------------------------------------------------
// debug taps: copy a named intermediate (channels-last, padded pitch) into the caller's buffer in the reference's (B, C, L) layout
// ------------------------------------------------------------------------------------------------
extern "C" int hificar_debug_tap(hificar_handle* h, const char* name, float* dst, size_t capacity) {
    if (!h) return fail(HIFICAR_E_INVALID, "null handle");
    h->taps.set(name, dst, capacity);
    return HIFICAR_OK;
}

// Test aid: every launch_conv launch of this engine takes tile shape (mi, wm, wn, ks, nb) — one of kTileCfgs — where tile_admissible lets it, and
// the planner's own choice elsewhere; mi = 0 gives every launch back to the planner.  Drops all plans, so the next launch of every shape is planned anew.
extern "C" int hificar_debug_force_tile(hificar_engine* e, int mi, int wm, int wn, int ks, int nb) {
    if (!e) return fail(HIFICAR_E_INVALID, "null engine");
    if (mi != 0) {
        bool known = false;
        for (const TileCfg& t : kTileCfgs) known = known || (t.MI == mi && t.WM == wm && t.WN == wn && t.KS == ks && t.NB == nb);
        if (!known) return fail(HIFICAR_E_INVALID, "hificar_debug_force_tile: (%d, %d, %d, %d, %d) is not a tile shape of the engine", mi, wm, wn, ks, nb);
    }
    const int rc = evict_plans(e);
    if (rc != HIFICAR_OK) return rc;
    const int req[5] = {mi, mi ? wm : 0, mi ? wn : 0, mi ? ks : 0, mi ? nb : 0};
    memcpy(e->force_tile, req, sizeof(req));
    return HIFICAR_OK;
}

static int emit_tap(hificar_handle* h, const std::string& name, const void* src, int pitch, int c0, int C, int nseq, int rows, int split,
                    hipStream_t stream, int src_rows = 0) {
    const size_t need = (size_t)nseq * C * rows;
    float* dst;
    const int rc = h->taps.find(name, need, &dst);
    if (rc != HIFICAR_OK || !dst) return rc;
    TapParams tp;
    tp.src = src;
    tp.dst = dst;
    tp.pitch = pitch;
    tp.c0 = c0;
    tp.C = C;
    tp.rows = rows;
    tp.src_rows = src_rows ? src_rows : rows;
    tp.total = (long long)need;
    tp.split = split;
    const unsigned blocks = (unsigned)std::min<long long>((tp.total + 255) / 256, 4096);
    hipLaunchKernelGGL(tap_copy_kernel, dim3(blocks), dim3(256), 0, stream, tp);
    HIP_TRY(hipGetLastError());
    return HIFICAR_OK;
}

static bool tap_wanted(const hificar_handle* h, const std::string& name) { return h->taps.wanted(name); }

// The `x0..x3, nin` prefix of the parameter blocks whose kernels average up to four fp32 streams (MrfSplitParams, PhHeadParams, OutConvParams
// and their backward blocks)
template <class P>
static void fill_inputs(P& p, const float* const* fin, int nin) {
    p.x0 = fin[0];
    p.x1 = nin > 1 ? fin[1] : nullptr;
    p.x2 = nin > 2 ? fin[2] : nullptr;
    p.x3 = nin > 3 ? fin[3] : nullptr;
    p.nin = nin;
}

// n branches of `rows` rows as launch_conv launches of layers l1 (io) or, with iop, as launch_pair launches of (l1, l2).  A launch carries up
// to three branches (MultiConvParams / PairParams): a fourth residual block rides in a second launch
static int launch_n(hificar_engine* h, const ConvLayer* const* l1, const ConvLayer* const* l2, int n, int nseq, int rows, const ConvIO* io,
                    const PairIOB* iop, float slope, const Ragged& rg, hipStream_t stream) {
    for (int q0 = 0; q0 < n; q0 += 3) {
        const int m = std::min(3, n - q0);
        const int r = iop ? launch_pair(h, l1 + q0, l2 + q0, m, nseq, rows, iop + q0, slope, rg, stream)
                          : launch_conv(h, l1 + q0, m, nseq, rows, io + q0, slope, rg, stream);
        if (r != HIFICAR_OK) return r;
    }
    return HIFICAR_OK;
}

// residual blocks of a stage run side by side, heaviest kernel size first
struct BlockOrder {
    int order[kMaxBlk];
    int max_d = 0;  // dilations of the deepest block
};
static BlockOrder block_order(const hificar_config& cfg) {
    BlockOrder bo;
    for (int j = 0; j < kMaxBlk; ++j) bo.order[j] = j;
    std::sort(bo.order, bo.order + cfg.n_blocks, [&](int a, int b) { return cfg.resblock_kernel_sizes[a] > cfg.resblock_kernel_sizes[b]; });
    for (int j = 0; j < cfg.n_blocks; ++j) bo.max_d = std::max(bo.max_d, cfg.n_dilations[j]);
    return bo;
}

// The branches of the launches of dilation d in one stage, in launch order: the blocks that have a dilation d, as block j[q] and the
// index ci[q] of its layer in convs1 / convs2
struct Branches {
    int n = 0;
    int j[kMaxBlk], ci[kMaxBlk];
};
static Branches gather_branches(const hificar_handle* h, const BlockOrder& bo, int stage, int d) {
    Branches br;
    for (int oj = 0; oj < h->cfg.n_blocks; ++oj) {
        const int j = bo.order[oj];
        if (d >= h->cfg.n_dilations[j]) continue;
        br.j[br.n] = j;
        br.ci[br.n] = conv_index(h, stage, j, d);
        ++br.n;
    }
    return br;
}

// LeakyReLU(0.01) + Conv1d(C -> 1, k) + tanh on the mean of `nin` fp32 inputs (hifigan.py:146-159, 231; gblock_gen.py:71-93, 131)
static int launch_output_conv(hificar_handle* h, const FwdCall& k, const Ragged& rg, const float* const* fin, int nin, int Cpad, int rows) {
    const hificar_config& cfg = h->cfg;
    OutConvParams op;
    memset(&op, 0, sizeof(op));
    fill_inputs(op, fin, nin);
    op.w = h->d_out_w;
    op.bias = h->out_bias;
    op.bias_ptr = h->d_out_bias;
    op.out = k.out;
    op.out_bstride = k.out_bstride;
    op.L = rows;
    op.C = Cpad;
    op.K = cfg.kernel_size;
    op.slope = 0.01f;
    op.use_tanh = cfg.use_tanh;
    op.seq_len = rg.seq_len;
    op.len_const = rg.seq_len ? -1 : rg.const_len;
    op.len_f0 = rg.f0;
    op.len_max = k.T;
    op.len_mul = rows / k.T;
    op.slots = k.slots;
    op.ctx = rg.ctx;
    op.ar_input = cfg.ar_input;
    op.hop = h->hop;
    // samples per workgroup: 256, or what a 64-KB LDS tile of (TR + K - 1) rows x (C + 1) floats + the weights allows
    const long long fit = ((long long)64 * 1024 / 4 - (long long)op.K * op.C) / (op.C + 1) - (op.K - 1);
    if (fit < 1) return fail(HIFICAR_E_INVALID, "output conv: %d channels x kernel %d does not fit the LDS tile", op.C, op.K);
    op.TR = (int)std::min<long long>(256, fit);
    const size_t lds = ((size_t)(op.TR + op.K - 1) * (op.C + 1) + (size_t)op.K * op.C) * sizeof(float);
    {
        const double pos = (double)k.B * rows;
        ProfScope prof(h, k.stream, "output_conv_kernel", 2.0 * pos * op.C * op.K, 4.0 * pos * (op.C * nin + 1));
        hipLaunchKernelGGL(output_conv_kernel, dim3((rows + op.TR - 1) / op.TR, k.B), dim3(256), lds, k.stream, op);
    }
    HIP_TRY(hipGetLastError());
    return HIFICAR_OK;
}

// Scratch for the pre-activation copies a debug tap wants and the normal path never writes: grown to `elems` floats
static int grow_tap_scratch(hificar_handle* h, size_t elems) {
    if (elems <= h->tap_scratch_elems) return HIFICAR_OK;
    if (h->tap_scratch) HIP_TRY(hipFree(h->tap_scratch));
    h->tap_scratch = nullptr;
    h->tap_scratch_elems = 0;
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, elems * sizeof(float)));
    h->tap_scratch = static_cast<float*>(p);
    h->tap_scratch_elems = elems;
    return HIFICAR_OK;
}

// What the steps of one HiFi-GAN forward hand on to each other
struct FwdState {
    Ragged rg;
    BlockOrder bo;
    int rows = 0;               // rows per sequence at the current stage
    const float* fin[kMaxBlk];  // where each branch's ResBlock output of the current stage lives
    const char* mrf_act = nullptr;  // the current stage's last ResBlock launch summed the branches (launch_merged): the ACTIVATED MRF mean, and fin is not written
    bool tapping = false;
    bool tap_convs1 = false;    // a conv1 output is wanted: those pairs run layer by layer (the fused kernel keeps it in LDS)
    size_t tap_se = 0;
};

// GBlockGenerator body of a forward: input conv -> GBlocks -> output conv (hificar_gblock.hip.inc)
static int gblock_forward(hificar_handle* h, const FwdCall& k, const Ragged& rg);

// 1. front end: the input rows of the input conv from the features, the PastFCEncoder of the AR context and the conditioning
static int launch_front(hificar_handle* h, const FwdCall& k) {
    const hificar_config& cfg = h->cfg;
    FrontParams fp;
    memset(&fp, 0, sizeof(fp));
    fp.c = k.c;
    fp.c_bstride = k.c_bstride;
    fp.c_cstride = k.c_cstride;
    fp.prev = k.prev;
    fp.prev_bstride = k.prev_bstride;
    fp.slots = k.slots;
    fp.valid = k.seq_len;
    if (k.ctx) {
        fp.prev = k.ctx;
        fp.prev_bstride = cfg.ar_input;
        fp.seqs = k.seqs;
        fp.seqs_slots = k.seqs_slots;
        fp.seqs_valid = k.seqs_valid;
    }
    fp.hop = h->hop;
    const bool f32 = h->precision == HIFICAR_PREC_F32;
    fp.xin = f32 ? (k.tp ? k.tp->xin : k.ws.xin) : nullptr;
    fp.xin_s = f32 ? nullptr : reinterpret_cast<char*>(k.ws.xin);
    fp.mlp_tape = k.tp ? k.tp->mlp : nullptr;
    fp.T = k.T;
    fp.t_valid = k.T_valid;
    if (cfg.use_spk_id) {
        fp.spk_id = k.spk_id;
        fp.spk_emb = h->d_spk_emb;
        fp.spk_w = h->d_spk_w;
        fp.spk_b = h->d_spk_b;
        fp.spk_e = cfg.spk_emb_size;
    }
    if (cfg.use_ph) {
        fp.ph = k.ph;
        fp.ph_stride = k.ph_stride;
        fp.ph_emb = h->d_ph_emb;
        fp.ph_e = cfg.ph_emb_size;
    }
    fp.cf = h->cf;
    fp.cin_pad = h->cin_pad;
    fp.use_ar = cfg.use_ar;
    fp.ar_input = cfg.ar_input;
    fp.ar_hidden = cfg.ar_hidden;
    fp.ar_output = cfg.ar_output;
    for (int l = 0; l < 5; ++l) {
        fp.wt[l] = h->d_mlp_w[l];
        fp.bs[l] = h->d_mlp_b[l];
    }
    {
        const double mlp_macs = cfg.use_ar ? (double)cfg.ar_input * cfg.ar_hidden + 3.0 * cfg.ar_hidden * cfg.ar_hidden +
                                                 (double)cfg.ar_hidden * cfg.ar_output : 0.0;
        ProfScope prof(h, k.stream, "front_kernel", 2.0 * k.B * mlp_macs, 4.0 * k.B * (mlp_macs + (double)k.T * (h->cf + h->cin_pad)));
        hipLaunchKernelGGL(front_kernel, dim3(k.B), dim3(kFrontThreads), 0, k.stream, fp);
    }
    HIP_TRY(hipGetLastError());
    return HIFICAR_OK;
}

// Activations travel between layers already activated — split rows (bf16x3) or plain fp32 rows (exact fp32), the
// "_s" buffers — and are staged by LDS-DMA; the layer's own fp32 value only where a residual / the MRF mean needs it
static char* act_h0(const FwdCall& k) { return k.tp ? k.tp->h0_s : reinterpret_cast<char*>(k.ws.h0); }
static char* act_xt(const FwdCall& k, int j) { return reinterpret_cast<char*>(k.ws.xt[j]); }

// 2. input conv (no activation in front of it: hifigan.py:221); its consumer applies LeakyReLU(slope)
static int forward_input_conv(hificar_handle* h, const FwdCall& k, const FwdState& fs) {
    const hificar_config& cfg = h->cfg;
    int rc;
    const ConvLayer* lay[1] = {&h->input_conv};
    float* y_tap = tap_wanted(h, "input_conv") ? h->tap_scratch + kMaxBlk * fs.tap_se : nullptr;
    const ConvIO io[1] = {{reinterpret_cast<char*>(k.tp ? k.tp->xin : k.ws.xin), nullptr, y_tap, act_h0(k)}};
    if ((rc = launch_conv(h, lay, 1, k.B, k.T, io, cfg.lrelu_slope, fs.rg, k.stream)) != HIFICAR_OK) return rc;
    if (y_tap && (rc = emit_tap(h, "input_conv", y_tap, stage_pad(cfg, 0), 0, cfg.channels, k.B, k.T, 0, k.stream)) != HIFICAR_OK) return rc;
    return HIFICAR_OK;
}

// The activated MRF mean of the previous stage's ResBlock outputs as its own launch -> the rows the upsampler reads
static int launch_mrf_split(hificar_handle* h, const FwdCall& k, const FwdState& fs, int i, const char** up_in) {
    const hificar_config& cfg = h->cfg;
    const int nbk = cfg.n_blocks;
    MrfSplitParams mq;
    memset(&mq, 0, sizeof(mq));
    fill_inputs(mq, fs.fin, nbk);
    mq.out = fs.fin[0] == k.ws.xt[0] ? k.ws.x_s[0] : act_xt(k, 0);  // a buffer none of the inputs lives in
    if (k.tp) mq.out = k.tp->upin_s[i];
    mq.C = stage_pad(cfg, i);
    mq.rows = (long long)k.B * fs.rows;
    mq.slope = cfg.lrelu_slope;
    mq.f32 = h->precision == HIFICAR_PREC_F32 ? 1 : 0;
    const long long units = mq.rows * (mq.C / 8);
    const unsigned blocks = (unsigned)std::min<long long>((units + 255) / 256, 8LL * h->num_cus);
    {
        ProfScope prof(h, k.stream, "mrf_split_kernel", 0.0, 4.0 * mq.rows * mq.C * (nbk + 1));
        hipLaunchKernelGGL(mrf_split_kernel, dim3(blocks), dim3(256), 0, k.stream, mq);
    }
    HIP_TRY(hipGetLastError());
    *up_in = mq.out;
    return HIFICAR_OK;
}

// debug taps of the residual stream of block j of stage i after dilation d
static int tap_block(hificar_handle* h, const FwdCall& k, const FwdState& fs, int i, int j, int d, const float* xcur) {
    if (!fs.tapping) return HIFICAR_OK;
    const hificar_config& cfg = h->cfg;
    const int Cs = stage_channels(cfg, i + 1), Cp = stage_pad(cfg, i + 1);
    const std::string base = "blocks." + std::to_string(i * cfg.n_blocks + j);
    int r = emit_tap(h, base + ".x." + std::to_string(d), xcur, Cp, 0, Cs, k.B, fs.rows, 0, k.stream);
    if (r == HIFICAR_OK && d + 1 == cfg.n_dilations[j]) r = emit_tap(h, base, xcur, Cp, 0, Cs, k.B, fs.rows, 0, k.stream);
    return r;
}

// ResBlock layers of a narrow stage whose every layer pair runs in the fused kernel: the residual stream stays fp32-only (the pair
// kernel activates + splits its input while staging), ping-ponging between x[j] and xt[j]; no activated copies
// are written at all.
static int resblocks_all_pairs(hificar_handle* h, const FwdCall& k, FwdState& fs, int i) {
    const hificar_config& cfg = h->cfg;
    const Workspace& ws = k.ws;
    const int nbk = cfg.n_blocks;
    int rc;
    const float* cur_f[kMaxBlk] = {ws.u, ws.u, ws.u, ws.u};
    for (int d = 0; d < fs.bo.max_d; ++d) {  // residual_block.py:217-221
        const ConvLayer* l1[kMaxBlk];
        const ConvLayer* l2[kMaxBlk];
        PairIOB iop[kMaxBlk];
        const Branches br = gather_branches(h, fs.bo, i, d);
        for (int n = 0; n < br.n; ++n) {
            const int j = br.j[n];
            l1[n] = &h->convs1[br.ci[n]];
            l2[n] = &h->convs2[br.ci[n]];
            // a tile's output pass must not overwrite rows a neighbouring tile still reads as halo: out != in
            float* out_f = cur_f[j] == ws.x[j] ? ws.xt[j] : ws.x[j];
            iop[n] = {cur_f[j], nullptr, cur_f[j], out_f, nullptr};
            cur_f[j] = out_f;
        }
        if ((rc = launch_n(h, l1, l2, br.n, k.B, fs.rows, nullptr, iop, cfg.lrelu_slope, fs.rg, k.stream)) != HIFICAR_OK) return rc;
        for (int j = 0; j < nbk; ++j)
            if (d < cfg.n_dilations[j] && (rc = tap_block(h, k, fs, i, j, d, cur_f[j])) != HIFICAR_OK) return rc;
    }
    for (int j = 0; j < nbk; ++j) fs.fin[j] = cur_f[j];
    return HIFICAR_OK;
}

// Whether stage i's last ResBlock launch may sum the branches (launch_merged) as far as the call decides it: exact fp32 inference without tape or taps
// (a tap wants the blocks' own outputs), not the last stage (the output conv and the phoneme head read the blocks' outputs), two blocks or more that
// all end at the same dilation, conv2 layers.  Off with HIFICAR_PAIR=0 (layer by layer: no fused launch forms), with HIFICAR_KSPLIT=0 (the batch-invariant
// mode: one accumulation order at every launch size — whether the merged form runs depends on the size, and it rounds differently), with
// HIFICAR_KSPLIT=2 (every launch split-K: the merged form has no such variant) and with HIFICAR_MRF_MERGE=0.  The rest — the pair of that dilation does not fuse, the planner's estimate — is resblocks_general's, at the launch.
static bool mrf_merge_allowed(const hificar_handle* h, const FwdCall& k, const FwdState& fs, int i) {
    const hificar_config& cfg = h->cfg;
    if (h->precision != HIFICAR_PREC_F32 || k.tp || fs.tapping || i + 1 >= cfg.n_stages || cfg.n_blocks < 2 || !cfg.use_additional_convs) return false;
    if (h->mrf_merge == 0 || !h->use_pair || h->ksplit != 1) return false;  // (HIFICAR_KSPLIT=2, "always split-K": the merged form is dense)
    for (int j = 0; j < cfg.n_blocks; ++j)
        if (cfg.n_dilations[j] != fs.bo.max_d) return false;
    return true;
}

// ResBlock layers of any other stage: activated copies ("_s") travel next to the fp32 stream; a dilation's pairs still fuse where they all can.
// u_act: the upsampler's activated output
static int resblocks_general(hificar_handle* h, const FwdCall& k, FwdState& fs, int i, const char* u_act) {
    const hificar_config& cfg = h->cfg;
    const Workspace& ws = k.ws;
    const Tape* const tp = k.tp;
    const int nbk = cfg.n_blocks, B = k.B, rows = fs.rows;
    const int Cs = stage_channels(cfg, i + 1), Cp = stage_pad(cfg, i + 1);
    const bool add_convs = cfg.use_additional_convs != 0;  // false: a ResBlock layer is x = x + conv1(LeakyReLU(x)) (residual_block.py:217-221)
    int rc;
    // fp32 residual streams; training keeps the LAST stage's (the output conv's backward needs the MRF mean) in the tape
    float* xres[kMaxBlk] = {ws.x[0], ws.x[1], ws.x[2], ws.x[3]};
    if (tp && i + 1 == cfg.n_stages)
        for (int j = 0; j < nbk; ++j) xres[j] = tp->fin[j];
    for (int j = 0; j < nbk; ++j) fs.fin[j] = xres[j];
    // activated stream of each branch: where the next conv1 reads its input.  It alternates between x_s[j] and
    // xt_s[j]: a launch never writes the buffer it (or a neighbouring tile, through the halo) reads.
    const char* cur_s[kMaxBlk] = {u_act, u_act, u_act, u_act};
    const bool may_merge = mrf_merge_allowed(h, k, fs, i);
    for (int d = 0; d < fs.bo.max_d; ++d) {  // residual_block.py:217-221
        const ConvLayer* l1[kMaxBlk];
        const ConvLayer* l2[kMaxBlk];
        ConvIO io1[kMaxBlk], io2[kMaxBlk];
        PairIOB iop[kMaxBlk];
        char* pair_out[kMaxBlk];
        char* lbl_out[kMaxBlk];
        bool fuse = add_convs;
        const Branches br = gather_branches(h, fs.bo, i, d);
        for (int n = 0; n < br.n; ++n) {
            const int j = br.j[n];
            char* const xt_s = act_xt(k, j);
            l1[n] = &h->convs1[br.ci[n]];
            l2[n] = add_convs ? &h->convs2[br.ci[n]] : nullptr;
            fuse = fuse && !fs.tap_convs1 && !tp && pair_eligible(h, *l1[n], *l2[n], B, rows);
            const bool last = d + 1 == cfg.n_dilations[j];
            // fused pair: cur -> the other buffer.  Layer by layer: cur -> mid -> the buffer that is not mid.
            pair_out[n] = cur_s[j] == ws.x_s[j] ? xt_s : ws.x_s[j];
            char* mid = cur_s[j] == xt_s ? ws.x_s[j] : xt_s;
            lbl_out[n] = mid == xt_s ? ws.x_s[j] : xt_s;
            if (tp) {  // training: unique buffers, kept for the backward pass
                mid = tp->xt_s[i][j][d];
                lbl_out[n] = tp->x_s[i][j][d];
            }
            io1[n] = {cur_s[j], nullptr, fs.tap_convs1 ? h->tap_scratch + (size_t)n * fs.tap_se : nullptr, mid};
            io2[n] = {mid, d == 0 ? ws.u : xres[j], xres[j], last ? nullptr : lbl_out[n]};
            if (!add_convs) {  // one conv per layer: conv1 carries the residual epilogue; its activated output is the next layer's input
                char* nxt = tp ? tp->x_s[i][j][d] : pair_out[n];
                io1[n] = {cur_s[j], d == 0 ? ws.u : xres[j], xres[j], last ? nullptr : nxt};
                lbl_out[n] = nxt;
            }
            iop[n] = {nullptr, cur_s[j], d == 0 ? ws.u : xres[j], xres[j], last ? nullptr : pair_out[n]};
        }
        if (fuse) {
            if ((rc = launch_n(h, l1, l2, br.n, B, rows, nullptr, iop, cfg.lrelu_slope, fs.rg, k.stream)) != HIFICAR_OK) return rc;
        } else {
            if ((rc = launch_n(h, l1, nullptr, br.n, B, rows, io1, nullptr, cfg.lrelu_slope, fs.rg, k.stream)) != HIFICAR_OK) return rc;
            if (add_convs && fs.tap_convs1)
                for (int q = 0; q < br.n; ++q)
                    if ((rc = emit_tap(h, "blocks." + std::to_string(i * nbk + br.j[q]) + ".convs1." + std::to_string(d), io1[q].y, Cp, 0, Cs,
                                       B, rows, 0, k.stream)) != HIFICAR_OK)
                        return rc;
            // the stage's last launch: all blocks summed in one accumulator, the activated MRF mean as the only output (launch_merged) — into
            // branch 0's free ping-pong buffer, which no launch reads any more — where the plan's estimate (or HIFICAR_MRF_MERGE=2) says so
            const ConvPlan* mpl = nullptr;
            if (may_merge && d + 1 == fs.bo.max_d && br.n == nbk) {
                if (!(mpl = get_plan(h, l2, nullptr, br.n, B, rows, 1, k.stream, &rc, true))) return rc;
                if (!mpl->merge_wins && h->mrf_merge != 2) mpl = nullptr;
            }
            if (mpl) {
                if ((rc = launch_merged(h, mpl, l2, br.n, B, rows, io2, lbl_out[0], cfg.lrelu_slope, fs.rg, k.stream)) != HIFICAR_OK) return rc;
                fs.mrf_act = lbl_out[0];
            } else if (add_convs && (rc = launch_n(h, l2, nullptr, br.n, B, rows, io2, nullptr, cfg.lrelu_slope, fs.rg, k.stream)) != HIFICAR_OK) return rc;
        }
        for (int q = 0; q < br.n; ++q)
            if ((rc = tap_block(h, k, fs, i, br.j[q], d, xres[br.j[q]])) != HIFICAR_OK) return rc;
        for (int q = 0; q < br.n; ++q) cur_s[br.j[q]] = fuse ? pair_out[q] : lbl_out[q];
    }
    return HIFICAR_OK;
}

// 3. one HiFi-GAN stage: MRF mean of the stage before -> upsampler -> ResBlocks side by side.  fs.rows / fs.fin: this stage's on return
static int forward_stage(hificar_handle* h, const FwdCall& k, FwdState& fs, int i) {
    const hificar_config& cfg = h->cfg;
    const Tape* const tp = k.tp;
    const int nbk = cfg.n_blocks;
    int rc;
    const char* up_in = act_h0(k);
    // MRF mean of the previous stage (hifigan.py:226-230).  Exact fp32 inference: folded into the upsampler's staging (ConvIO::x_more — its
    // loader waves read the blocks' fp32 streams, sum, divide, activate), so no launch and no buffer for the mean exist.  Training (the tape keeps
    // the activated mean for the upsampler's weight gradient) and bf16x3 (split rows): mrf_split_kernel.
    // Where the previous stage's last launch summed the blocks itself (launch_merged) the upsampler reads that one activated stream by LDS-DMA.
    const char* const merged_in = fs.mrf_act;
    fs.mrf_act = nullptr;
    const bool fold_mrf = i > 0 && h->precision == HIFICAR_PREC_F32 && !tp && !merged_in;
    if (merged_in) up_in = merged_in;
    if (i > 0 && !fold_mrf && !merged_in && (rc = launch_mrf_split(h, k, fs, i, &up_in)) != HIFICAR_OK) return rc;
    // Whether every layer pair of the stage runs in the fused kernel (resblocks_all_pairs) or not (resblocks_general)
    bool all_pairs = !fs.tap_convs1 && !tp && cfg.use_additional_convs != 0;
    for (int j = 0; j < nbk && all_pairs; ++j)
        for (int d = 0; d < cfg.n_dilations[j]; ++d) {
            const int ci = conv_index(h, i, j, d);
            all_pairs = all_pairs && pair_eligible(h, h->convs1[ci], h->convs2[ci], k.B, fs.rows * cfg.upsample_scales[i]);
        }
    char* const u_act = tp ? tp->u_s[i] : k.ws.u_s;
    {   // LeakyReLU + ConvTranspose1d (hifigan.py:224): fp32 u (first residual) (+ activated copy: first conv input)
        const ConvLayer* lay[1] = {&h->ups[i]};
        ConvIO io[1] = {{up_in, nullptr, k.ws.u, all_pairs ? nullptr : u_act}};
        if (fold_mrf) {
            io[0].xs = reinterpret_cast<const char*>(fs.fin[0]);
            io[0].x_slope = cfg.lrelu_slope;
            io[0].x_n = nbk;
            for (int j = 1; j < nbk; ++j) io[0].x_more[j - 1] = fs.fin[j];
        }
        if ((rc = launch_conv(h, lay, 1, k.B, fs.rows, io, cfg.lrelu_slope, fs.rg, k.stream)) != HIFICAR_OK) return rc;
    }
    fs.rows *= cfg.upsample_scales[i];
    if (fs.tapping && (rc = emit_tap(h, "upsamples." + std::to_string(i), k.ws.u, stage_pad(cfg, i + 1), 0, stage_channels(cfg, i + 1), k.B, fs.rows, 0,
                                     k.stream)) != HIFICAR_OK)
        return rc;
    return all_pairs ? resblocks_all_pairs(h, k, fs, i) : resblocks_general(h, k, fs, i, u_act);
}

// phoneme-loss head on the last stage's MRF mean (hifigan.py:232-237)
static int launch_ph_head(hificar_handle* h, const FwdCall& k, const FwdState& fs) {
    const hificar_config& cfg = h->cfg;
    const int nbk = cfg.n_blocks;
    PhHeadParams pq;
    memset(&pq, 0, sizeof(pq));
    fill_inputs(pq, fs.fin, nbk);
    pq.w = h->d_phfc_w;
    pq.bias = h->d_phfc_b;
    pq.out = k.ph_out;
    pq.C = stage_channels(cfg, cfg.n_stages);
    pq.Cp = stage_pad(cfg, cfg.n_stages);
    pq.L = fs.rows;
    pq.T = k.ph_out_T;
    pq.hop = h->hop;
    pq.num_ph = cfg.num_ph;
    pq.seq_len = k.seq_len;
    pq.len_const = k.seq_len ? -1 : (k.T_valid < k.T ? k.T_valid : -1);
    ProfScope prof(h, k.stream, "ph_head_kernel", 2.0 * k.B * k.T_valid * (double)pq.C * cfg.num_ph, 4.0 * k.B * (double)fs.rows * pq.Cp * nbk);
    hipLaunchKernelGGL(ph_head_kernel, dim3(k.T_valid, k.B), dim3(256), 0, k.stream, pq);
    HIP_TRY(hipGetLastError());
    return HIFICAR_OK;
}

// One generator forward: every generator path ends here.
static int forward_impl(hificar_handle* h, FwdCall k) {
    const hificar_config& cfg = h->cfg;
    if (k.T_valid < 0) k.T_valid = k.T;
    FwdState fs;
    fs.rg = ragged_of(k);
    int rc;
    if ((rc = launch_front(h, k)) != HIFICAR_OK) return rc;
    if (h->arch == 1) return gblock_forward(h, k, fs.rg);

    fs.bo = block_order(cfg);
    fs.rows = k.T;
    for (int j = 0; j < kMaxBlk; ++j) fs.fin[j] = k.ws.x[j];
    fs.tapping = !h->taps.empty();
    if (fs.tapping) {
        const bool f32 = h->precision == HIFICAR_PREC_F32;
        fs.tap_convs1 = h->taps.any_contains(".convs1.");
        fs.tap_se = stage_elems(h, k.B, k.T);
        // pre-activation copies that the normal path never writes: 3 stage-sized scratch buffers
        if ((rc = grow_tap_scratch(h, kMaxBlk * fs.tap_se + (size_t)k.B * k.T * stage_pad(cfg, 0))) != HIFICAR_OK) return rc;
        if (cfg.use_ar && (rc = emit_tap(h, "ar_feats", k.ws.xin, f32 ? h->cin_pad : -h->cin_pad, h->cf, cfg.ar_output, k.B, 1, f32 ? 0 : 1, k.stream, k.T)) != HIFICAR_OK)
            return rc;
    }
    if ((rc = forward_input_conv(h, k, fs)) != HIFICAR_OK) return rc;
    for (int i = 0; i < cfg.n_stages; ++i)
        if ((rc = forward_stage(h, k, fs, i)) != HIFICAR_OK) return rc;
    if (cfg.use_ph_loss && k.ph_out && (rc = launch_ph_head(h, k, fs)) != HIFICAR_OK) return rc;
    // 4. output conv: LeakyReLU(0.01) + Conv1d + tanh (hifigan.py:146-159)
    return launch_output_conv(h, k, fs.rg, fs.fin, cfg.n_blocks, stage_pad(cfg, cfg.n_stages), fs.rows);
}

// The record of a forward over whole utterances of T frames: (B, cf, T) features, (B, ar_input) AR context, (B, hop T) waveform; T and ws: the caller
static FwdCall whole_call(const hificar_handle* h, const float* c, const float* ar, const int32_t* spk_id, const int32_t* ph, float* out, float* ph_out,
                          int B, int T, hipStream_t stream) {
    FwdCall k;
    k.c = c;
    k.c_bstride = (int64_t)h->cf * T;
    k.c_cstride = T;
    k.prev = h->cfg.use_ar ? ar : nullptr;
    k.prev_bstride = h->cfg.ar_input;
    k.out = out;
    k.out_bstride = (int64_t)h->hop * T;
    k.B = B;
    k.T_valid = T;
    k.spk_id = spk_id;
    k.ph = ph;
    k.ph_stride = T;
    k.ph_out = ph_out;
    k.ph_out_T = T;
    k.stream = stream;
    return k;
}

static int check_ready(hificar_handle* h, int B, int T, void* ws, size_t ws_bytes) {
    if (!h) return fail(HIFICAR_E_INVALID, "null handle");
    if (!h->finalized) return fail(HIFICAR_E_STATE, "hificar_finalize has not been called");
    if (B < 1 || T < 1) return fail(HIFICAR_E_INVALID, "B=%d, T=%d must be positive", B, T);
    const size_t need = hificar_workspace_bytes(h, B, T);
    if (!ws || ws_bytes < need) return fail(HIFICAR_E_WORKSPACE, "workspace too small: need %zu bytes, got %zu", need, ws_bytes);
    if ((reinterpret_cast<uintptr_t>(ws) & 255) != 0) return fail(HIFICAR_E_INVALID, "workspace must be 256-byte aligned");
    return HIFICAR_OK;
}

extern "C" int hificar_forward_cond(hificar_handle* h, const float* c, const float* ar, const int32_t* spk_id, const int32_t* ph,
                                    const int32_t* lengths, float* out, float* ph_out, int B, int T, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    int rc = check_ready(h, B, T, workspace, workspace_bytes);
    if (rc != HIFICAR_OK) return rc;
    if (!c || !out) return fail(HIFICAR_E_INVALID, "hificar_forward: null tensor");
    if (h->cfg.use_ar && !ar) return fail(HIFICAR_E_INVALID, "use_ar model needs the ar context (got NULL)");
    if (h->cfg.use_spk_id && !spk_id) return fail(HIFICAR_E_INVALID, "use_spk_id model needs spk_id (got NULL)");
    if (h->cfg.use_ph && !ph) return fail(HIFICAR_E_INVALID, "use_ph model needs ph (got NULL)");
    if ((rc = enter_stream(h, static_cast<hipStream_t>(stream))) != HIFICAR_OK) return rc;
    FwdCall k = whole_call(h, c, ar, spk_id, ph, out, ph_out, B, T, static_cast<hipStream_t>(stream));
    k.T = bucket_frames(T);
    k.seq_len = lengths;
    k.ws = plan_workspace(h, B, k.T, workspace);
    return forward_impl(h, k);
}

extern "C" int hificar_forward_ragged(hificar_handle* h, const float* c, const float* ar, const int32_t* lengths, float* out, int B,
                                      int T, void* workspace, size_t workspace_bytes, void* stream) {
    if (h && (h->cfg.use_spk_id || h->cfg.use_ph))
        return fail(HIFICAR_E_INVALID, "this model takes spk_id / ph: call hificar_forward_cond");
    return hificar_forward_cond(h, c, ar, nullptr, nullptr, lengths, out, nullptr, B, T, workspace, workspace_bytes, stream);
}

extern "C" int hificar_forward(hificar_handle* h, const float* c, const float* ar, float* out, int B, int T, void* workspace,
                               size_t workspace_bytes, void* stream) {
    return hificar_forward_ragged(h, c, ar, nullptr, out, B, T, workspace, workspace_bytes, stream);
}

// The first checks of every *_cond AR entry point: the model runs autoregressively (who_ar names the family in that refusal), and each
// conditioning pointer is there exactly when the model uses it.
static int check_ar_model(const hificar_handle* h, const char* who_ar, const char* who, const void* spk, const void* ph) {
    if (!h->cfg.use_ar) return fail(HIFICAR_E_INVALID, "%s on a model built with use_ar=false", who_ar);
    if (h->cfg.use_spk_id && !spk) return fail(HIFICAR_E_INVALID, "%s: use_spk_id model needs spk_id (got NULL)", who);
    if (h->cfg.use_ph && !ph) return fail(HIFICAR_E_INVALID, "%s: use_ph model needs ph (got NULL)", who);
    if (!h->cfg.use_spk_id && spk) return fail(HIFICAR_E_INVALID, "%s: spk_id given to a model built with use_spk_id=false", who);
    if (!h->cfg.use_ph && ph) return fail(HIFICAR_E_INVALID, "%s: ph given to a model built with use_ph=false", who);
    return HIFICAR_OK;
}

// A loop of more than one chunk feeds the last ar_input samples of a chunk's audio to the next chunk
static int check_ar_chunk(const hificar_handle* h, int chunk_frames, bool more_chunks) {
    if (h->cfg.ar_input > h->hop * chunk_frames && more_chunks)
        return fail(HIFICAR_E_INVALID, "ar_input (%d) > chunk audio length (%d): the reference loop (decode.py:79-81) is ill-formed there",
                    h->cfg.ar_input, h->hop * chunk_frames);
    return HIFICAR_OK;
}

static int check_lengths(const int32_t* lengths_host, int n, int T_max) {
    for (int b = 0; b < n; ++b)
        if (lengths_host[b] < 0 || lengths_host[b] > T_max)
            return fail(HIFICAR_E_INVALID, "lengths[%d]=%d outside [0, %d]", b, lengths_host[b], T_max);
    return HIFICAR_OK;
}

// The record of chunk f0 of hificar_ar_loop for the Bn utterances from b0 on of a batch of (B, cf, T_total) features and (B, hop T_total) audio
static FwdCall ar_chunk_call(const hificar_handle* h, const float* c, const int32_t* spk_id, const int32_t* ph, float* out, int T_total, int chunk_frames,
                             int f0, int b0, int Bn, void* workspace, hipStream_t stream) {
    FwdCall k;
    k.c_bstride = (int64_t)h->cf * T_total;
    k.c_cstride = T_total;
    k.prev_bstride = k.out_bstride = (int64_t)h->hop * T_total;
    const int64_t pos = b0 * k.out_bstride + (int64_t)h->hop * f0;
    k.c = c + (size_t)b0 * h->cf * T_total + f0;
    // prev = last ar_input samples already written for this utterance (zeros for the first chunk)
    k.prev = f0 == 0 ? nullptr : out + pos - h->cfg.ar_input;
    k.out = out + pos;
    k.B = Bn;
    k.T = std::min(chunk_frames, T_total - f0);
    k.f0 = f0;
    // chunk f0 of utterance b reads spk_id[b] and ph[b, f0 + t]
    k.spk_id = spk_id ? spk_id + b0 : nullptr;
    k.ph = ph ? ph + (size_t)b0 * T_total + f0 : nullptr;
    k.ph_stride = T_total;
    k.ws = plan_workspace(h, Bn, k.T, workspace);
    k.stream = stream;
    return k;
}

// The loop of a mid-size batch on TWO streams (round 4).  Utterances do not depend on each other, and a step is a chain of 34 dependent launches whose tile
// lists quantise badly between batch 17 and 62 (a 25-frame chunk is ONE 128-row tile per utterance at the widest stage: 6 B tiles of weight
// 11 : 7 : 3 for 256 workgroups — batch 44 to 64 all take the same 11 units): the two halves of the batch run their own chains on two streams
// and each half's idle workgroups, launch latencies and tails are filled by the other half's kernels.  Measured (10-s clips, chunk 25, fp32,
// single / dual ms per step): batch 18 108.2 / 103.4, 22 130.3 / 122.6, 28 146.3 / 135.3, 32 153.1 / 142.2, 36 184.6 / 171.3, 44 224.8 / 201.5,
// 48 225.4 / 214.7, 56 263.7 / 239.2, 60 266.2 / 258.8; below the window the halves' launches are less efficient than the whole batch's
// (batch 8: 58.1 / 68.1, 4: 44.2 / 48.4, 16: 90.7 / 91.6), at 64 the tile lists are full (269.3 / 276.5).  Same kernels, same per-utterance
// arithmetic up to the launch-shape dependence HIFICAR_KSPLIT=0 removes.  Not while profiling or tapping (one stream's events / scratch), not for
// ragged batches (their steps shrink the batch prefix).
// ws0_bytes: the first half's workspace; the second half's follows it.
static int ar_loop_two_streams(hificar_handle* h, const float* c, const int32_t* spk_id, const int32_t* ph, float* out, int B, int T_total,
                               int chunk_frames, void* workspace, size_t ws0_bytes, hipStream_t s0) {
    if (!h->ar_side) {
        HIP_TRY(hipStreamCreateWithFlags(&h->ar_side, hipStreamNonBlocking));
        for (hipEvent_t& e : h->ar_ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    const hipStream_t s1 = h->ar_side;
    HIP_TRY(hipEventRecord(h->ar_ev[0], s0));  // fork: the side stream starts behind the caller's work so far
    HIP_TRY(hipStreamWaitEvent(s1, h->ar_ev[0], 0));
    // The halves' launches share the chip, so a launch's own exact makespan is the wrong yardstick for its tile shape (measured: with the
    // simulated makespan the halves pick shapes that fill the chip alone and batch 32 / 44 lose 5 / 4 %; choosing by workgroup-time as the
    // discriminators' engine does loses 20-30 %): they keep the closed-form estimate.  (Reset below on every path: nothing in between returns.)
    h->shared_chip = true;
    unsigned long long seen = h->sched_up_seq;
    // a tile schedule first needed by one half is uploaded on that half's stream: the other stream must not use it before it has landed
    auto publish = [&](hipStream_t from, hipStream_t to, hipEvent_t ev) -> int {
        if (h->sched_up_seq != seen) {
            HIP_TRY(hipEventRecord(ev, from));
            HIP_TRY(hipStreamWaitEvent(to, ev, 0));
            seen = h->sched_up_seq;
        }
        return HIFICAR_OK;
    };
    const int B0 = (B + 1) / 2;  // the second half's rows start at B0, its workspace behind the first half's
    char* const wsp1 = static_cast<char*>(workspace) + ws0_bytes;
    int rc = HIFICAR_OK;
    for (int f0 = 0; f0 < T_total && rc == HIFICAR_OK; f0 += chunk_frames) {
        rc = forward_impl(h, ar_chunk_call(h, c, spk_id, ph, out, T_total, chunk_frames, f0, 0, B0, workspace, s0));
        if (rc == HIFICAR_OK) rc = publish(s0, s1, h->ar_ev[0]);
        if (rc == HIFICAR_OK) rc = forward_impl(h, ar_chunk_call(h, c, spk_id, ph, out, T_total, chunk_frames, f0, B0, B - B0, wsp1, s1));
        if (rc == HIFICAR_OK) rc = publish(s1, s0, h->ar_ev[1]);
    }
    h->shared_chip = false;
    // join (also on an error return: the caller's stream must stay ordered behind what the side stream was given)
    if (hipEventRecord(h->ar_ev[1], s1) != hipSuccess || hipStreamWaitEvent(s0, h->ar_ev[1], 0) != hipSuccess)
        return rc != HIFICAR_OK ? rc : fail(HIFICAR_E_HIP, "hificar_ar_loop: joining the side stream failed");
    return rc;
}

extern "C" int hificar_ar_loop_cond(hificar_handle* h, const float* c, const int32_t* spk_id, const int32_t* ph, const int32_t* lengths,
                                    const int32_t* lengths_host, float* out, int B, int T_total, int chunk_frames, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    int rc;
    if (h && (rc = check_ar_model(h, "hificar_ar_loop", "hificar_ar_loop", spk_id, ph)) != HIFICAR_OK) return rc;
    if (chunk_frames < 1) return fail(HIFICAR_E_INVALID, "chunk_frames=%d must be positive", chunk_frames);
    if ((rc = check_ready(h, B, std::min(chunk_frames, std::max(T_total, 1)), workspace, workspace_bytes)) != HIFICAR_OK) return rc;
    if (T_total < 1) return fail(HIFICAR_E_INVALID, "T_total=%d must be positive", T_total);
    if (!c || !out) return fail(HIFICAR_E_INVALID, "hificar_ar_loop: null tensor");
    if ((rc = check_ar_chunk(h, chunk_frames, T_total > chunk_frames)) != HIFICAR_OK) return rc;
    const hipStream_t s0 = static_cast<hipStream_t>(stream);
    if ((rc = enter_stream(h, s0)) != HIFICAR_OK) return rc;
    if (lengths_host && !lengths) return fail(HIFICAR_E_INVALID, "hificar_ar_loop_ragged: lengths_host without the device copy");
    if (lengths_host && (rc = check_lengths(lengths_host, B, T_total)) != HIFICAR_OK) return rc;
    const int Tn_max = std::min(chunk_frames, T_total);
    const size_t ws0_bytes = plan_workspace(h, (B + 1) / 2, Tn_max, nullptr).bytes;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(s0, &cap);  // (a loop being captured into a hipGraph stays on the capturing stream)
    if (!lengths && B >= 2 && B >= h->ar_dual_min && B <= h->ar_dual_max && !h->profiling && h->taps.empty() && cap == hipStreamCaptureStatusNone &&
        ws0_bytes + plan_workspace(h, B / 2, Tn_max, nullptr).bytes <= workspace_bytes)
        return ar_loop_two_streams(h, c, spk_id, ph, out, B, T_total, chunk_frames, workspace, ws0_bytes, s0);
    for (int f0 = 0; f0 < T_total; f0 += chunk_frames) {
        // With the host copy of the lengths the step only covers the utterances still running: the batch prefix up to the
        // last one longer than f0 (all of them when the batch is sorted longest first).
        int Bn = B;
        if (lengths_host) {
            Bn = 0;
            for (int b = 0; b < B; ++b)
                if (lengths_host[b] > f0) Bn = b + 1;
            if (Bn == 0) break;
        }
        FwdCall k = ar_chunk_call(h, c, spk_id, ph, out, T_total, chunk_frames, f0, 0, Bn, workspace, s0);
        k.seq_len = lengths;
        if ((rc = forward_impl(h, k)) != HIFICAR_OK) return rc;
    }
    return HIFICAR_OK;
}

extern "C" int hificar_ar_loop_ragged(hificar_handle* h, const float* c, const int32_t* lengths, const int32_t* lengths_host,
                                      float* out, int B, int T_total, int chunk_frames, void* workspace, size_t workspace_bytes,
                                      void* stream) {
    // (a model built with use_ar=false is refused by hificar_ar_loop_cond, as its first check)
    if (h && h->cfg.use_ar && (h->cfg.use_spk_id || h->cfg.use_ph))  // the reference's ar_loop calls model(c, ar=prev) only (decode.py:72)
        return fail(HIFICAR_E_INVALID, "hificar_ar_loop: speaker / phoneme conditioned models are driven through hificar_forward_cond");
    return hificar_ar_loop_cond(h, c, nullptr, nullptr, lengths, lengths_host, out, B, T_total, chunk_frames, workspace, workspace_bytes, stream);
}

// The step table of the packed loop: steps[s] = {sequences, frames} of step s, whose row of `slots` lists the utterances it advances as
// (utterance, first frame) and whose row of `valid` their valid frames.  Rows start on an even index in both arrays.
struct PackedSteps {
    struct Step {
        int n, frames;
    };
    std::vector<Step> steps;
    std::vector<int2> slots;
    std::vector<int> valid;
};
static PackedSteps packed_step_table(const int32_t* lengths_host, int N, int T_max, int chunk_frames, int batch) {
    PackedSteps t;
    std::vector<int> run, f0((size_t)N, 0);
    int next = 0;
    for (;;) {
        while ((int)run.size() < batch && next < N) {
            if (lengths_host[next] > 0) run.push_back(next);
            ++next;
        }
        if (run.empty()) break;
        // every step is launched over a full chunk (shorter last chunks are masked per sequence and their empty tiles
        // skipped): launch shapes then differ by the number of running utterances only, and their schedules stay cached
        t.steps.push_back({(int)run.size(), std::min(chunk_frames, T_max)});
        for (int u : run) {
            t.slots.push_back(int2{u, f0[u]});
            t.valid.push_back(std::min(chunk_frames, lengths_host[u] - f0[u]));
        }
        t.slots.resize((t.slots.size() + 1) & ~(size_t)1);  // rows start on an even index in both arrays (int2 rows 16-byte aligned)
        t.valid.resize(t.slots.size());
        std::vector<int> keep;
        for (int u : run) {
            f0[u] += chunk_frames;
            if (f0[u] < lengths_host[u]) keep.push_back(u);
        }
        run.swap(keep);
    }
    return t;
}

// Packed (continuously batched) AR synthesis: N utterances, at most `batch` of them in flight; as soon as one finishes the
// next one takes its place, so every step but the last few runs a full batch whatever the lengths are.  The AR state of
// an utterance is its own waveform so far, so a "slot" exists only in the host-side step table uploaded here.
extern "C" int hificar_ar_loop_packed_cond(hificar_handle* h, const float* c, const int32_t* spk_id, const int32_t* ph,
                                           const int32_t* lengths_host, float* out, int N, int T_max, int chunk_frames, int batch,
                                           void* workspace, size_t workspace_bytes, void* stream_) {
    int rc;
    if (h && (rc = check_ar_model(h, "hificar_ar_loop", "hificar_ar_loop_packed", spk_id, ph)) != HIFICAR_OK) return rc;
    if (chunk_frames < 1 || batch < 1 || N < 1 || T_max < 1)
        return fail(HIFICAR_E_INVALID, "hificar_ar_loop_packed: N=%d, T_max=%d, chunk_frames=%d, batch=%d must be positive", N, T_max,
                    chunk_frames, batch);
    batch = std::min(batch, N);
    if ((rc = check_ready(h, batch, std::min(chunk_frames, T_max), workspace, workspace_bytes)) != HIFICAR_OK) return rc;
    if (!c || !out || !lengths_host) return fail(HIFICAR_E_INVALID, "hificar_ar_loop_packed: null argument");
    if ((rc = check_ar_chunk(h, chunk_frames, T_max > chunk_frames)) != HIFICAR_OK) return rc;
    if ((rc = check_lengths(lengths_host, N, T_max)) != HIFICAR_OK) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if ((rc = enter_stream(h, stream)) != HIFICAR_OK) return rc;
    const PackedSteps tab = packed_step_table(lengths_host, N, T_max, chunk_frames, batch);
    if (tab.steps.empty()) return HIFICAR_OK;
    const size_t n_slots = tab.slots.size(), tab_bytes = n_slots * (sizeof(int2) + sizeof(int));
    if (!h->tab_copied) HIP_TRY(hipEventCreateWithFlags(&h->tab_copied, hipEventDisableTiming));
    else HIP_TRY(hipEventSynchronize(h->tab_copied));  // the previous upload has left the staging copy (long ago, normally)
    if (tab_bytes > h->tab_bytes) {
        if (h->d_tab) HIP_TRY(hipFree(h->d_tab));  // synchronises: no earlier call can still be reading it
        if (h->h_tab) HIP_TRY(hipHostFree(h->h_tab));
        h->d_tab = h->h_tab = nullptr;
        h->tab_bytes = 0;
        HIP_TRY(hipMalloc(&h->d_tab, tab_bytes * 2));
        HIP_TRY(hipHostMalloc(&h->h_tab, tab_bytes * 2, hipHostMallocDefault));
        h->tab_bytes = tab_bytes * 2;
    }
    int2* d_slots = static_cast<int2*>(h->d_tab);
    int* d_valid = reinterpret_cast<int*>(d_slots + n_slots);
    memcpy(h->h_tab, tab.slots.data(), n_slots * sizeof(int2));
    memcpy(static_cast<char*>(h->h_tab) + n_slots * sizeof(int2), tab.valid.data(), tab.valid.size() * sizeof(int));
    // one asynchronous upload, ordered on the stream behind any earlier call that still reads the table
    HIP_TRY(hipMemcpyAsync(h->d_tab, h->h_tab, tab_bytes, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(h->tab_copied, stream));
    FwdCall k;  // the features and the conditioning are indexed by utterance / (utterance, frame) through the slots
    k.c = c;
    k.c_bstride = (int64_t)h->cf * T_max;
    k.c_cstride = T_max;
    k.prev = k.out = out;
    k.prev_bstride = k.out_bstride = (int64_t)h->hop * T_max;
    k.spk_id = spk_id;
    k.ph = ph;
    k.ph_stride = T_max;
    k.stream = stream;
    size_t row = 0;
    for (const PackedSteps::Step& st : tab.steps) {
        k.B = st.n;
        k.T = st.frames;
        k.seq_len = d_valid + row;
        k.slots = d_slots + row;
        k.ws = plan_workspace(h, st.n, st.frames, workspace);
        if ((rc = forward_impl(h, k)) != HIFICAR_OK) return rc;
        row += ((size_t)st.n + 1) & ~(size_t)1;
    }
    return HIFICAR_OK;
}

extern "C" int hificar_ar_loop_packed(hificar_handle* h, const float* c, const int32_t* lengths_host, float* out, int N, int T_max,
                                      int chunk_frames, int batch, void* workspace, size_t workspace_bytes, void* stream) {
    // (a model built with use_ar=false is refused by hificar_ar_loop_packed_cond, as its first check)
    if (h && h->cfg.use_ar && (h->cfg.use_spk_id || h->cfg.use_ph))  // the reference's ar_loop calls model(c, ar=prev) only (decode.py:72)
        return fail(HIFICAR_E_INVALID, "hificar_ar_loop: speaker / phoneme conditioned models are driven through hificar_forward_cond");
    return hificar_ar_loop_packed_cond(h, c, nullptr, nullptr, lengths_host, out, N, T_max, chunk_frames, batch, workspace, workspace_bytes, stream);
}

extern "C" int hificar_ar_loop(hificar_handle* h, const float* c, float* out, int B, int T_total, int chunk_frames,
                               void* workspace, size_t workspace_bytes, void* stream) {
    return hificar_ar_loop_ragged(h, c, nullptr, nullptr, out, B, T_total, chunk_frames, workspace, workspace_bytes, stream);
}

// One step of the AR loop for n sessions whose context outlives the call (streaming synthesis).  It is the packed loop's step in
// context mode: the same launches over a full chunk, short last chunks masked per sequence on the device, the AR input read from /
// written back to the caller's context arena by front_kernel / output_conv_kernel (FrontParams::seqs, OutConvParams::ctx).  The step
// table is written into a ring of mapped pinned slots that front_kernel reads where they are (an upload would put a DMA transfer in
// front of every step's launches), so the host never waits for earlier steps unless kStepRing of them are queued.
static constexpr int kStepRing = 32;
extern "C" int hificar_ar_step_cond(hificar_handle* h, const float* c, int64_t c_bstride, int64_t c_cstride, const int32_t* spk_rows,
                                    const int32_t* ph, int64_t ph_bstride, const int32_t* seqs_host, int n, int chunk_frames, float* ctx,
                                    int ctx_rows, float* out, void* workspace, size_t workspace_bytes, void* stream_) {
    // every argument is checked before the handle's state (finalize, workspace): nothing is enqueued for a bad table
    if (!h) return fail(HIFICAR_E_INVALID, "null handle");
    int rc;
    if ((rc = check_ar_model(h, "hificar_ar_step", "hificar_ar_step", spk_rows, ph)) != HIFICAR_OK) return rc;
    if (ph && (ph_bstride < 1 || ph_bstride > INT32_MAX))
        return fail(HIFICAR_E_INVALID, "hificar_ar_step: phoneme ring row pitch %lld outside [1, 2^31)", (long long)ph_bstride);
    if (n < 1 || chunk_frames < 1 || ctx_rows < 1)
        return fail(HIFICAR_E_INVALID, "hificar_ar_step: n=%d, chunk_frames=%d, ctx_rows=%d must be positive", n, chunk_frames, ctx_rows);
    if (!c || !seqs_host || !ctx || !out) return fail(HIFICAR_E_INVALID, "hificar_ar_step: null argument");
    if ((rc = check_ar_chunk(h, chunk_frames, true)) != HIFICAR_OK) return rc;
    if (c_bstride < 0 || c_cstride < 1) return fail(HIFICAR_E_INVALID, "hificar_ar_step: strides %lld / %lld", (long long)c_bstride, (long long)c_cstride);
    if (n > ctx_rows) return fail(HIFICAR_E_INVALID, "hificar_ar_step: %d sequences for %d context rows", n, ctx_rows);
    std::vector<char> seen((size_t)ctx_rows, 0);
    bool all_full = true;
    for (int b = 0; b < n; ++b) {
        const int32_t* e = seqs_host + 4 * (size_t)b;
        if (e[0] < 0 || e[0] >= ctx_rows) return fail(HIFICAR_E_INVALID, "hificar_ar_step: sequence %d: row %d outside [0, %d)", b, e[0], ctx_rows);
        if (seen[(size_t)e[0]]) return fail(HIFICAR_E_INVALID, "hificar_ar_step: row %d appears twice in one step", e[0]);
        seen[(size_t)e[0]] = 1;
        if (e[2] < 1 || e[2] > chunk_frames)
            return fail(HIFICAR_E_INVALID, "hificar_ar_step: sequence %d: valid frames %d outside [1, %d]", b, e[2], chunk_frames);
        all_full = all_full && e[2] == chunk_frames;
        if (e[1] < 0 || (int64_t)e[1] + e[2] > c_cstride)
            return fail(HIFICAR_E_INVALID, "hificar_ar_step: sequence %d: frames [%d, %d) outside the feature rows (%lld)", b, e[1], e[1] + e[2],
                        (long long)c_cstride);
        if (ph && (int64_t)e[1] + e[2] > ph_bstride)
            return fail(HIFICAR_E_INVALID, "hificar_ar_step: sequence %d: frames [%d, %d) outside the phoneme ring's rows (%lld)", b, e[1],
                        e[1] + e[2], (long long)ph_bstride);
    }
    if ((rc = check_ready(h, n, chunk_frames, workspace, workspace_bytes)) != HIFICAR_OK) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if ((rc = enter_stream(h, stream)) != HIFICAR_OK) return rc;
    const size_t cap = ((size_t)ctx_rows + 1) & ~(size_t)1;  // entries: any valid table of this arena fits (n <= ctx_rows)
    if (cap > h->step_cap) {
        for (auto& st : h->step_ring)  // the old slots may still be read by queued steps
            if (st.used) HIP_TRY(hipEventSynchronize(st.done));
        if (h->step_d) HIP_TRY(hipFree(h->step_d));
        if (h->step_h) HIP_TRY(hipHostFree(h->step_h));
        h->step_d = h->step_h = h->step_hd = nullptr;
        h->step_cap = 0;
        HIP_TRY(hipMalloc(&h->step_d, cap * (sizeof(int2) + sizeof(int))));
        HIP_TRY(hipHostMalloc(&h->step_h, cap * sizeof(int4) * kStepRing, hipHostMallocMapped | hipHostMallocCoherent));
        HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&h->step_hd), h->step_h, 0));
        h->step_cap = cap;
        h->step_ring.resize(kStepRing);
        for (auto& st : h->step_ring) {
            if (!st.done) HIP_TRY(hipEventCreateWithFlags(&st.done, hipEventDisableTiming));
            st.used = false;
        }
    }
    const unsigned k = h->step_next++ % kStepRing;
    auto& slot = h->step_ring[k];
    if (slot.used) HIP_TRY(hipEventSynchronize(slot.done));  // fired long ago unless kStepRing steps are queued
    int4* hs = reinterpret_cast<int4*>(h->step_h) + (size_t)k * h->step_cap;
    for (int b = 0; b < n; ++b) {
        const int32_t* e = seqs_host + 4 * (size_t)b;
        hs[b] = int4{e[0], e[1], e[2], e[3] != 0};
    }
    // the device table front_kernel publishes: slots (row, frame) | valid frames (int2 rows 16-byte aligned: cap is even).  One copy
    // serves every step: a step's launches are done with it before the next step's front_kernel runs (one stream, enter_stream)
    int2* d_slots = reinterpret_cast<int2*>(h->step_d);
    int* d_valid = reinterpret_cast<int*>(d_slots + h->step_cap);
    FwdCall fc;
    fc.c = c;
    fc.c_bstride = c_bstride;
    fc.c_cstride = c_cstride;
    fc.out = out;
    fc.out_bstride = (int64_t)h->hop * chunk_frames;
    fc.B = n;
    fc.T = chunk_frames;
    // a step of full chunks only (every step but a session's last) runs the launches unmasked, as an ar_synthesis step does: the masked
    // form's per-tile length loads cost ~1 us per launch, and for full chunks both forms compute the same values
    fc.seq_len = all_full ? nullptr : d_valid;
    fc.slots = d_slots;
    fc.ctx = ctx;
    fc.seqs = reinterpret_cast<const int4*>(h->step_hd) + (size_t)k * h->step_cap;
    fc.seqs_slots = d_slots;
    fc.seqs_valid = d_valid;
    fc.spk_id = spk_rows;  // one speaker per session row: front_kernel indexes both by the table's row
    fc.ph = ph;
    fc.ph_stride = (int)ph_bstride;
    fc.ws = plan_workspace(h, n, chunk_frames, workspace);
    fc.stream = stream;
    rc = forward_impl(h, fc);
    // (also behind a failed step: what it did enqueue may read the slot)
    if (hipEventRecord(slot.done, stream) == hipSuccess) slot.used = true;
    else if (rc == HIFICAR_OK) rc = fail(HIFICAR_E_HIP, "hificar_ar_step: recording the step's event failed");
    return rc;
}

extern "C" int hificar_ar_step(hificar_handle* h, const float* c, int64_t c_bstride, int64_t c_cstride, const int32_t* seqs_host, int n,
                               int chunk_frames, float* ctx, int ctx_rows, float* out, void* workspace, size_t workspace_bytes,
                               void* stream) {
    if (h && h->cfg.use_ar && (h->cfg.use_spk_id || h->cfg.use_ph))  // the reference's ar_loop calls model(c, ar=prev) only (decode.py:72)
        return fail(HIFICAR_E_INVALID, "hificar_ar_step: speaker / phoneme conditioned models are driven through hificar_forward_cond");
    return hificar_ar_step_cond(h, c, c_bstride, c_cstride, nullptr, nullptr, 0, seqs_host, n, chunk_frames, ctx, ctx_rows, out, workspace,
                                workspace_bytes, stream);
}

// ------------------------------------------------------------------------------------------------
// per-kernel event timing
// ------------------------------------------------------------------------------------------------
extern "C" hificar_engine* hificar_engine_of(hificar_handle* h) { return h; }

extern "C" int hificar_profile_begin(hificar_engine* h) {
    if (!h) return fail(HIFICAR_E_INVALID, "null handle");
    for (auto& r : h->prof) {
        (void)hipEventDestroy(r.e0);
        (void)hipEventDestroy(r.e1);
    }
    h->prof.clear();
    h->profiling = true;
    return HIFICAR_OK;
}

extern "C" int hificar_profile_end(hificar_engine* h, hificar_kernel_stat* stats, int max_stats, int* n_stats) {
    if (!h || !n_stats) return fail(HIFICAR_E_INVALID, "null argument");
    h->profiling = false;
    if (!h->prof.empty()) HIP_TRY(hipStreamSynchronize(h->prof_stream));
    std::vector<hificar_kernel_stat> agg;
    for (auto& r : h->prof) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, r.e0, r.e1));
        size_t k = 0;
        for (; k < agg.size(); ++k)
            if (r.name == agg[k].name) break;
        if (k == agg.size()) {
            hificar_kernel_stat st;
            memset(&st, 0, sizeof(st));
            snprintf(st.name, sizeof(st.name), "%s", r.name.c_str());
            agg.push_back(st);
        }
        agg[k].launches += 1;
        agg[k].total_ms += ms;
        agg[k].flops += r.flops;
        agg[k].bytes += r.bytes;
        (void)hipEventDestroy(r.e0);
        (void)hipEventDestroy(r.e1);
    }
    h->prof.clear();
    std::sort(agg.begin(), agg.end(), [](const hificar_kernel_stat& a, const hificar_kernel_stat& b) { return a.total_ms > b.total_ms; });
    *n_stats = (int)agg.size();
    for (int i = 0; i < (int)agg.size() && i < max_stats && stats; ++i) stats[i] = agg[i];
    return HIFICAR_OK;
}

extern "C" int hificar_pcm16(const float* x, int16_t* y, size_t n, void* stream) {
    if (!x || !y) return fail(HIFICAR_E_INVALID, "hificar_pcm16: null pointer");
    if (n == 0) return HIFICAR_OK;
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(pcm16_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), x, y, n);
    HIP_TRY(hipGetLastError());
    return HIFICAR_OK;
}

#include "hificar_train.hip.inc"
#include "hificar_gblock.hip.inc"
#include "hificar_disc.hip.inc"
#include "hificar_mel.hip.inc"
#include "hificar_feat.hip.inc"

// ------------------------------------------------------------------------------------------------
// What the training states of the two feature models (BiGRU, Transformer) share: the table of their device-resident parameters — every
// float tensor of the state_dict in one master copy, the trainable ones in front, in gradient-buffer order — and its hand-over.
// ------------------------------------------------------------------------------------------------

struct FeatureParamTable {
    struct Slot {
        std::string name;
        std::vector<int64_t> shape;
        int64_t offset, numel;
    };
    std::vector<Slot> slots;                // the trainable parameters in gradient-buffer order (reference names and layouts)
    std::map<std::string, int64_t> offset;  // name -> floats into the master copy (the trainable ones: = into the gradient buffer)
    int64_t grad_total = 0;                 // floats of the gradient buffer
    int64_t master_total = 0;               // ... of the master copy: the tensors and, behind them, the model's derived forms (its folds)
    float* d_master = nullptr;

    // the next tensor of the master copy, at a multiple of four floats
    void add(const FeatureShapes& expected, const std::string& name, bool trainable) {
        const std::vector<int64_t>& shape = expected.at(name);
        int64_t n = 1;
        for (auto v : shape) n *= v;
        offset[name] = master_total;
        if (trainable) slots.push_back({name, shape, master_total, n});
        master_total += (n + 3) & ~(int64_t)3;
    }
    // `floats` of the master copy behind what it holds so far, for a derived form
    int64_t reserve(int64_t floats) {
        const int64_t at = master_total;
        master_total += floats;
        return at;
    }
    float* at(const std::string& name) const { return d_master + offset.at(name); }
};

// hificar_{bigru,xfmr}_grad_info
static int feature_grad_info(const FeatureParamTable& tab, int i, char* name96, int64_t* offset, int64_t* numel) {
    if (i < 0 || i >= (int)tab.slots.size()) return fail(HIFICAR_E_INVALID, "gradient index %d out of range", i);
    const FeatureParamTable::Slot& s = tab.slots[(size_t)i];
    snprintf(name96, 96, "%s", s.name.c_str());
    *offset = s.offset;
    *numel = s.numel;
    return HIFICAR_OK;
}

// hificar_{bigru,xfmr}_set_parameters_device (`what`) up to the master copy: n device tensors, every name of `expected` exactly once.  Every
// name is checked before any byte is copied: a refused list leaves the master copy, and with it the handle, exactly as it was.
static int feature_upload(const FeatureShapes& expected, const FeatureParamTable& tab, const char* const* names, const float* const* data, int n,
                          const char* what, hipStream_t stream) {
    if (n != (int)expected.size()) return fail(HIFICAR_E_INVALID, "%s: %d tensors, the model has %zu", what, n, expected.size());
    std::set<std::string> seen;
    for (int i = 0; i < n; ++i) {
        if (!names[i] || !data[i]) return fail(HIFICAR_E_INVALID, "%s: null entry %d", what, i);
        if (!expected.count(names[i])) return fail(HIFICAR_E_INVALID, "unexpected tensor name '%s' for this configuration", names[i]);
        if (!seen.insert(names[i]).second) return fail(HIFICAR_E_INVALID, "tensor '%s' given twice", names[i]);
    }
    for (int i = 0; i < n; ++i) {
        size_t numel = 1;
        for (auto v : expected.at(names[i])) numel *= (size_t)v;
        HIP_TRY(hipMemcpyAsync(tab.at(names[i]), data[i], numel * sizeof(float), hipMemcpyDeviceToDevice, stream));
    }
    return HIFICAR_OK;
}

// zeroed device memory on the engine's allocation list (freed with the handle)
static int feature_alloc(hificar_engine* h, size_t bytes, void** out) {
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, bytes));
    h->allocs.push_back(p);
    HIP_TRY(hipMemset(p, 0, bytes));
    *out = p;
    return HIFICAR_OK;
}

// rows of a training step's buffers for B x T frames: slack behind the last row for whole GEMM tiles
static size_t feature_train_rows(int B, int T) { return round_up_sz((size_t)B * (size_t)T + 64, 256); }

// The first training entry point on a handle builds its training state.  A failed set-up (out of device memory, in practice) is final for
// the handle: what it allocated stays on the engine's allocation list until destroy, so another attempt per entry point would only grow
// that list.  Nothing half-built stays behind.
template <class G, class TS>
static int feature_train_make(G* g, int (*build)(G*, TS*), const char* model) {
    if (g->train_failed != HIFICAR_OK)
        return fail(g->train_failed, "the %s training state could not be set up on this handle earlier; destroy it and make a new one", model);
    std::unique_ptr<TS> ts(new TS());
    const int rc = build(g, ts.get());
    if (rc != HIFICAR_OK) return g->train_failed = rc;
    g->train = ts.release();
    return HIFICAR_OK;
}

#include "hificar_bigru.hip.inc"
#include "hificar_bigru_train.hip.inc"
#include "hificar_xfmr.hip.inc"
#include "hificar_xfmr_train.hip.inc"
#include "hificar_hubert.hip.inc"
#include "hificar_linear.hip.inc"
