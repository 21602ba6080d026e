/*
 * hificar.h — C ABI of libhificar.so: the MI355X-native (gfx950) HiFi-GAN / HiFi-CAR generator
 * forward pass (200-Hz EMA/pitch frames -> 16-kHz waveform).
 *
 * The reference (articulatory/articulatory) has NO native boundary for this path: it is a Python
 * class protocol on top of PyTorch operators.  Each entry point below therefore names the
 * reference Python interface it stands in for (paths relative to the reference repo):
 *
 *   hificar_create          HiFiGANGenerator.__init__            articulatory/models/hifigan.py:24-196
 *   hificar_gblock_create   GBlockGenerator.__init__             articulatory/models/gblock_gen.py:17-109 (forward :111-132 = hificar_forward*)
 *   hificar_set_weight      load_state_dict + remove_weight_norm articulatory/utils/utils.py:340-342,
 *                                                                articulatory/models/hifigan.py:256-266
 *   hificar_finalize        model.eval().to(device)              egs/ema/voc1/local/predict_wav.py:114-115
 *   hificar_forward         HiFiGANGenerator.forward             articulatory/models/hifigan.py:198-239
 *   hificar_forward_cond    ... with spk_id= / ph= and the (out, ph_out) return of use_ph_loss    hifigan.py:212-220, 232-237
 *   hificar_ar_loop         ar_loop (non-WSOLA branch), batched  articulatory/bin/decode.py:31-83
 *   hificar_forward_ragged  the per-utterance loop over a dataset calling .inference()  egs/ema/voc1/local/predict_wav.py:124-137,
 *   hificar_ar_loop_ragged  ... or ar_loop(), one utterance at a time                    articulatory/bin/decode.py:292-351
 *                           (a batch of utterances of DIFFERENT lengths in one call; results per utterance are those of
 *                           the one-at-a-time loop, bit for bit)
 *   hificar_ar_loop_packed  the same dataset loop, continuously batched (a finished utterance's place is taken by the next)
 *   hificar_ar_step         one chunk of ar_loop (decode.py:54-83) for each of n live sessions; the AR context  articulatory/bin/decode.py:54-83
 *                           (prev = cout[:, :, -ar_input:], decode.py:77-78) persists between calls in a caller-owned arena
 *   hificar_ar_loop_cond, hificar_ar_loop_packed_cond, hificar_ar_step_cond
 *                           the same three loops for speaker- / phoneme-conditioned models: every chunk's forward is
 *                           forward(c, spk_id=, ar=prev, ph=)                    articulatory/bin/decode.py:54-83 + hifigan.py:212-220
 *   hificar_bigru_*         BiGRU (the speech-to-EMA inversion model): __init__, load_state_dict, eval().to(device), forward
 *                                                                articulatory/models/pytorch_models.py:22-72 (declared at the end of this file)
 *   hificar_xfmr_*          Transformer (the feature-to-feature encoder): __init__, load_state_dict, eval().to(device), forward
 *                                                                articulatory/models/transformer.py:21-77 (declared at the end of this file)
 *   hificar_pcm16           sf.write(..., "PCM_16") sample conversion articulatory/bin/decode.py:319-324
 *   hificar_workspace_bytes (torch's caching allocator does this implicitly in the reference)
 *   hificar_last_error      Python exceptions / assert           articulatory/models/hifigan.py:78-80
 *
 * Conventions
 *   - plain pointers and sizes only; no torch types.  Device pointers are HIP device pointers.
 *   - tensors at the boundary use the reference's layouts: features (B, C, T) fp32 with T contiguous,
 *     AR context (B, 1, ar_input) fp32, waveform (B, 1, hop*T) fp32.
 *   - every function returns 0 on success or a negative HIFICAR_E_* code; hificar_last_error() then
 *     returns a thread-local, human-readable message.  Nothing ever calls exit().
 *   - all device work is enqueued on the caller-supplied hipStream_t (passed as void*); no call
 *     synchronises the device except hificar_finalize() (one-time weight upload) and the FIRST call for a new
 *     (batch, frames) shape, which builds and uploads that shape's tile schedules (small device allocations + blocking
 *     copies; cached in the handle afterwards, so a warm-up call per shape keeps the steady state fully asynchronous).
 *   - a handle is not thread-safe; use one handle per (process, device) and, from one host thread at a time, preferably ONE stream
 *     per handle.  The tile-schedule arenas, the packed AR loop's step table and the caller's workspace are shared state of the
 *     handle: every entry point that enqueues work first makes its stream wait (hipStreamWaitEvent on an event recorded on the
 *     previous call's stream) for everything earlier calls on this handle enqueued, so calls on DIFFERENT streams are serialised
 *     behind each other, never overlapped.  Concurrency comes from separate handles (each with its own workspace), not from streams.
 */
#ifndef HIFICAR_H
#define HIFICAR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIFICAR_MAX_STAGES 8
#define HIFICAR_MAX_BLOCKS 4
#define HIFICAR_MAX_DILATIONS 4

#define HIFICAR_OK 0
#define HIFICAR_E_INVALID (-1)     /* bad argument / unsupported hyper-parameter            */
#define HIFICAR_E_STATE (-2)       /* call order (e.g. forward before finalize, missing weight) */
#define HIFICAR_E_HIP (-3)         /* a HIP runtime call failed (message carries hipGetErrorString) */
#define HIFICAR_E_WORKSPACE (-4)   /* workspace too small                                    */

/* arithmetic used by the convolution kernels */
#define HIFICAR_PREC_F32 0         /* v_mfma_f32_32x32x2_f32: exact fp32 multiply, fp32 accumulate */
#define HIFICAR_PREC_BF16X3 1      /* fp32 operands split hi+lo bf16, 3 bf16 MFMAs, fp32 accumulate */
#define HIFICAR_PREC_BF16X3W 2     /* hificar_xfmr_set_train_precision ONLY: bf16x3, and the one-tap GEMM-form weight gradients in it too;
                                      every other entry point that takes a precision refuses it (HIFICAR_E_INVALID) */
#define HIFICAR_PREC_BF16X3A 3     /* hificar_xfmr_set_precision and hificar_hubert_set_precision ONLY: bf16x3, and the attention's products on
                                      bf16 MFMAs too (v_mfma_f32_16x16x32_bf16, hi hi + hi lo + lo hi, fp32 accumulate; inference only); every
                                      other entry point that takes a precision refuses it (HIFICAR_E_INVALID) */
#define HIFICAR_PREC_BF16X3WA 4    /* hificar_xfmr_set_train_precision ONLY: bf16x3w, and the training attention's query-tiled kernels (forward
                                      and backward-q: seven of its ten banded products) on v_mfma_f32_16x16x32_bf16 too; every other entry
                                      point that takes a precision refuses it (HIFICAR_E_INVALID) */
#define HIFICAR_PREC_BF16X3WAC 6   /* hificar_xfmr_set_train_precision ONLY: bf16x3wa, and the weight gradients of the wide k = 3 ResBlock convs
                                      as one-tap GEMMs on tap-shifted split columns (v_mfma_f32_32x32x16_bf16) too; every other entry point
                                      that takes a precision refuses it (HIFICAR_E_INVALID) */
#define HIFICAR_PREC_BF16X3WACK 8  /* hificar_xfmr_set_train_precision ONLY: bf16x3wac, and the attention's key-tiled backward (dK, dV and the
                                      first stage of the position tables' gradient) on v_mfma_f32_16x16x32_bf16 too; every other entry point
                                      that takes a precision refuses it (HIFICAR_E_INVALID).  5 and 7 are no arithmetic. */

typedef struct hificar_handle hificar_handle;
/* The conv engine every model of the library launches through (plans, schedules, stream ordering, profiling).  A generator handle
 * has one (hificar_engine_of), so do the discriminators (hificar_disc_engine), the BiGRU (hificar_bigru_engine), the Transformer (hificar_xfmr_engine), the speech features (hificar_feat_engine) and the HuBERT encoder (hificar_hubert_engine); it lives and
 * dies with its model.  Only the profiling calls take it: the generator's entry points do not accept another model's engine. */
typedef struct hificar_engine hificar_engine;

/* Mirrors the keyword arguments of HiFiGANGenerator.__init__ (hifigan.py:24-50) that affect
 * inference.  in_channels keeps the reference's meaning: feature dims + ar_output when use_ar. */
typedef struct hificar_config {
    int32_t in_channels;
    int32_t out_channels; /* must be 1 */
    int32_t channels;
    int32_t kernel_size;
    int32_t n_stages;
    int32_t upsample_scales[HIFICAR_MAX_STAGES];
    int32_t upsample_kernel_sizes[HIFICAR_MAX_STAGES];
    int32_t n_blocks;
    int32_t resblock_kernel_sizes[HIFICAR_MAX_BLOCKS];
    int32_t n_dilations[HIFICAR_MAX_BLOCKS];
    int32_t resblock_dilations[HIFICAR_MAX_BLOCKS][HIFICAR_MAX_DILATIONS];
    int32_t use_additional_convs; /* 0: a ResBlock layer is x + convs1[d](x) (residual_block.py:191-205, 217-221), no convs2 tensors */
    int32_t bias;                 /* ResBlock conv bias flag */
    float lrelu_slope;            /* nonlinear_activation_params.negative_slope */
    int32_t use_tanh;
    int32_t use_ar;
    int32_t ar_input;
    int32_t ar_hidden;
    int32_t ar_output;
    int32_t precision; /* HIFICAR_PREC_* */
    /* speaker / phoneme conditioning (hifigan.py:43-49, 176-189); all zero = off, as in every shipped YAML */
    int32_t use_spk_id;   /* adds spk_fc(spk_emb_mat[spk_id]) to every input channel of every frame (hifigan.py:212-216) */
    int32_t num_spk;
    int32_t spk_emb_size;
    int32_t use_ph;       /* appends ph_emb_mat[ph[b, t]] as ph_emb_size extra input channels (hifigan.py:217-220); in_channels counts them */
    int32_t num_ph;
    int32_t ph_emb_size;
    int32_t use_ph_loss;  /* second output: phoneme logits AvgPool1d(2*hop, hop, hop/2)(ph_fc(c)) at the frame rate (hifigan.py:232-237) */
} hificar_config;

/* Build an (empty) generator for these hyper-parameters on the current HIP device. */
int hificar_create(const hificar_config* cfg, hificar_handle** out);

/* The reference's OTHER a2w generator behind the same plugin surface: GBlockGenerator (articulatory/models/gblock_gen.py:14-132; GAN-TTS
 * style GBlocks, articulatory/layers/pytorch_layers.py:32-91).  Mirrors the keyword arguments of GBlockGenerator.__init__
 * (gblock_gen.py:17-31).  input conv (kernel_size) -> n_blocks GBlocks -> LeakyReLU(0.01) + conv (kernel_size) (+ tanh); GBlock i maps
 * channels / in_div[i] -> channels / out_div[i] channels with the reference's hard-coded plan in_div = 1,1,1,2,2,2,2,4,4,8,
 * out_div = 1,1,2,2,2,2,4,4,8,8 (gblock_gen.py:63-64) and upsamples by g_scales[i] (nearest neighbour):
 *     y = conv_k,d3(ReLU(conv_k(up(ReLU(x))))) + conv_1(up(x));   out = y + conv_k,d27(ReLU(conv_k,d9(ReLU(y))))
 * The handle is an ordinary hificar_handle: hificar_set_weight (names "input_conv.weight", "resamples.<i>.conv1.<1|2>.weight",
 * "resamples.<i>.conv1.<3|4>.weight", "resamples.<i>.res1.<0|1>.weight" (cout, cin, 1), "resamples.<i>.conv2.{1,3}.weight", the biases,
 * "output_conv.1.*", "ar_model.model.*", "spk_*" — the Sequential indices move by one when g_scales[i] > 1, as in the reference's
 * state_dict), hificar_finalize, hificar_forward[_cond / _ragged], hificar_ar_loop*, hificar_forward_train[_cond], hificar_backward[_cond],
 * hificar_set_parameters_device, ... all take it.  Exact-fp32 arithmetic only (res1 consumes the raw, un-activated rows).
 * Restrictions (each is a configuration the reference class itself cannot run, see oracle/make_golden_gblock.py): g_kernel_sizes odd;
 * the last GBlock must end at channels / 8 channels (n_blocks = 9 or 10). */
#define HIFICAR_MAX_GBLOCKS 10
typedef struct hificar_gblock_config {
    int32_t in_channels;  /* feature dims + ar_output when use_ar, as in hificar_config */
    int32_t out_channels; /* must be 1 */
    int32_t channels;
    int32_t kernel_size;  /* input / output conv */
    int32_t n_blocks;     /* len(g_scales) == len(g_kernel_sizes) */
    int32_t g_scales[HIFICAR_MAX_GBLOCKS];
    int32_t g_kernel_sizes[HIFICAR_MAX_GBLOCKS];
    int32_t use_tanh;
    int32_t use_ar;
    int32_t ar_input;
    int32_t ar_hidden;
    int32_t ar_output;
    int32_t use_spk_id;   /* gblock_gen.py:103-106, 123-127 */
    int32_t num_spk;
    int32_t spk_emb_size;
    int32_t precision;    /* must be HIFICAR_PREC_F32 */
} hificar_gblock_config;
int hificar_gblock_create(const hificar_gblock_config* cfg, hificar_handle** out);

/* Hand over one FOLDED tensor (weight-norm already baked: w = v*g/||v||) by its reference
 * state_dict name after remove_weight_norm(), e.g. "input_conv.weight", "upsamples.0.1.weight"
 * (Cin,Cout,K), "blocks.3.convs1.2.1.bias", "output_conv.1.weight", "ar_model.model.4.weight".
 * `data` is a HOST pointer to contiguous fp32 in the reference's layout; the library repacks into
 * its kernel layout and the caller keeps ownership. */
int hificar_set_weight(hificar_handle* h, const char* name, const float* data, const int64_t* shape, int ndim);

/* Check that every tensor arrived, repack, upload to the device.  Synchronises the device once. */
int hificar_finalize(hificar_handle* h);

/* Switch the conv arithmetic after creation (HIFICAR_PREC_*).  Cheap; weights for both modes are resident. */
int hificar_set_precision(hificar_handle* h, int precision);

/* Bytes of device scratch hificar_forward / hificar_ar_loop need for B utterances of T frames per call
 * (for hificar_ar_loop pass T = chunk_frames). */
size_t hificar_workspace_bytes(const hificar_handle* h, int B, int T);

/* One generator forward.  c: (B, in_channels - ar_output*use_ar, T) contiguous device fp32;
 * ar: (B, 1, ar_input) contiguous device fp32, or NULL when !use_ar; out: (B, 1, hop*T) device fp32,
 * hop = prod(upsample_scales).  Inputs are not modified. */
int hificar_forward(hificar_handle* h, const float* c, const float* ar, float* out, int B, int T,
                    void* workspace, size_t workspace_bytes, void* stream);

/* Batched autoregressive synthesis of B equal-length utterances (decode.py:54-83 per utterance):
 * c: (B, C, T_total) device fp32; out: (B, hop*T_total) device fp32.  Chunks of chunk_frames frames
 * (= batch_max_steps / hop_size, decode.py:50) run sequentially, each conditioned on the last ar_input
 * output samples of the previous one (zeros for the first); the last chunk may be shorter.
 * Requires ar_input <= hop*chunk_frames (the only case in which the reference's loop is well formed). */
int hificar_ar_loop(hificar_handle* h, const float* c, float* out, int B, int T_total, int chunk_frames,
                    void* workspace, size_t workspace_bytes, void* stream);

/* hificar_forward with the conditioning inputs of HiFiGANGenerator.forward(c, spk_id=, ar=, ph=) (hifigan.py:198-239):
 * spk_id: device pointer to B int32 speaker indices (use_spk_id) or NULL; ph: device pointer to (B, T) int32 phoneme indices
 * (use_ph) or NULL; ph_out: device pointer to (B, num_ph, T) fp32 (use_ph_loss: the reference then returns (out, ph_out)) or NULL.
 * lengths as in hificar_forward_ragged (NULL: all T).  Features c: (B, in_channels - ar_output*use_ar - ph_emb_size*use_ph, T). */
int hificar_forward_cond(hificar_handle* h, const float* c, const float* ar, const int32_t* spk_id, const int32_t* ph,
                         const int32_t* lengths, float* out, float* ph_out, int B, int T, void* workspace, size_t workspace_bytes,
                         void* stream);

/* Ragged batches: B utterances of different lengths, padded to a common T (T_total) in `c`.
 * lengths: DEVICE pointer to B int32 frame counts (0 <= lengths[b] <= T), or NULL (all T).  Utterance b is
 * synthesised exactly as if it were alone: frames >= lengths[b] do not exist for it (its convs see zero padding
 * there — also in the shorter last AR chunk, decode.py:56-58 — and nothing is written to out[b, hop*lengths[b]:],
 * which keeps whatever the caller put there).  This is the dataset loop of predict_wav.py:124-137 /
 * decode.py:292-351 run B utterances at a time. */
int hificar_forward_ragged(hificar_handle* h, const float* c, const float* ar, const int32_t* lengths, float* out, int B,
                           int T, void* workspace, size_t workspace_bytes, void* stream);
int hificar_ar_loop_ragged(hificar_handle* h, const float* c, const int32_t* lengths, const int32_t* lengths_host, float* out,
                           int B, int T_total, int chunk_frames, void* workspace, size_t workspace_bytes, void* stream);
/* lengths_host: optional HOST copy of the same B values (NULL = unknown to the host).  With it, every AR step is launched
 * only over the utterances still running — the batch prefix up to the last one longer than the step's first frame, i.e.
 * all of them and nothing else when the batch is sorted longest first — instead of masking finished ones on the device. */

/* Packed ("continuously batched") AR synthesis of a whole list of utterances: c (N, C, T_max) and out (N, hop*T_max) on the
 * device, lengths_host N frame counts on the HOST.  At most `batch` utterances are in flight; when one finishes, the next
 * one of the list takes its place in the following step, so all steps but the last few run a full batch whatever the
 * length distribution (list the utterances longest first for the shortest tail).  Per utterance the result is that of
 * hificar_ar_loop on it alone, bit for bit; out[u, hop*lengths[u]:] is left untouched.
 * workspace: hificar_workspace_bytes(h, batch, chunk_frames).  Stands in for the dataset loop of
 * articulatory/bin/decode.py:292-351 / egs/ema/voc1/local/predict_wav.py:124-137. */
int hificar_ar_loop_packed(hificar_handle* h, const float* c, const int32_t* lengths_host, float* out, int N, int T_max,
                           int chunk_frames, int batch, void* workspace, size_t workspace_bytes, void* stream);

/* Streaming synthesis: ONE step of the reference's AR loop (articulatory/bin/decode.py:54-83) for n sessions, each advancing by one chunk,
 * with the AR context of every session kept between calls in the caller's arena ctx: (ctx_rows, ar_input) device fp32, one row per
 * session.  seqs_host: n HOST rows of four int32 {row, frame, valid, first}:
 *   row    the session's context row in [0, ctx_rows), at most once per step; also its feature row in c
 *   frame  first frame of the chunk in c: element (row, ch, t) at c[row*c_bstride + ch*c_cstride + t]; frame + valid <= c_cstride
 *   valid  frames of this chunk, 1..chunk_frames (fewer: the session's last chunk, decode.py:56)
 *   first  nonzero: the session's first chunk — its AR input is zeros, whatever the row holds (no memset of a reused row needed)
 * out: (n, hop*chunk_frames) device fp32, dense by sequence; out[b, hop*valid:] is left untouched.  A full chunk also writes its
 * last ar_input samples into its ctx row, which the session's next step reads (decode.py:77-78).  Per session the concatenated
 * output is hificar_ar_loop's on the concatenated frames.  Launches exactly the kernels of one hificar_ar_loop step of n utterances
 * (one chunk), and no copy: the table goes into a ring of mapped pinned slots that the first kernel reads in place, so the call
 * does not wait for device work (unless 32 steps of this handle are still queued).  workspace: hificar_workspace_bytes(h, n, chunk_frames).  Requires use_ar, no speaker /
 * phoneme conditioning (hificar_ar_step_cond takes those), ar_input <= hop*chunk_frames; the table is checked on the host before anything is enqueued. */
int hificar_ar_step(hificar_handle* h, const float* c, int64_t c_bstride, int64_t c_cstride, const int32_t* seqs_host, int n,
                    int chunk_frames, float* ctx, int ctx_rows, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* The AR loops for speaker- / phoneme-conditioned models.  The reference's ar_loop calls model(cin, ar=prev_samples) only (decode.py:72)
 * and cannot run such a model; these entry points keep its chunking and feedback (articulatory/bin/decode.py:54-83) and make every chunk's
 * forward the reference's forward(c, spk_id=, ar=prev, ph=) (hifigan.py:212-220) with the utterance's own speaker and the chunk's slice of
 * its phoneme row, so an utterance's result is that of the one-at-a-time loop of hificar_forward_cond calls on its chunks (bit for bit
 * with HIFICAR_KSPLIT=0).  Waveform only: no ph_out (use_ph_loss models return the first output).  Each conditioning pointer is required
 * exactly when the model uses it (use_spk_id / use_ph) and must be NULL otherwise; with both NULL these ARE hificar_ar_loop_ragged /
 * _packed / hificar_ar_step.  The library reads the indices on the device and cannot check them: the CALLER guarantees
 * 0 <= spk_id < num_spk and 0 <= ph < num_ph for every element of the tensors described below (padding included). */

/* hificar_ar_loop_ragged with spk_id: device (B) int32, one speaker per utterance, and ph: device (B, T_total) int32, frame-aligned
 * with c (entries at or past lengths[b] are not used but must be valid indices).  decode.py:54-83 + hifigan.py:212-220. */
int hificar_ar_loop_cond(hificar_handle* h, const float* c, const int32_t* spk_id, const int32_t* ph, const int32_t* lengths,
                         const int32_t* lengths_host, float* out, int B, int T_total, int chunk_frames, void* workspace,
                         size_t workspace_bytes, void* stream);

/* hificar_ar_loop_packed with spk_id: device (N) int32 and ph: device (N, T_max) int32, indexed by utterance like c: a slot taken over
 * by the next utterance of the list takes that utterance's speaker and phonemes with it.  decode.py:54-83 + hifigan.py:212-220. */
int hificar_ar_loop_packed_cond(hificar_handle* h, const float* c, const int32_t* spk_id, const int32_t* ph, const int32_t* lengths_host,
                                float* out, int N, int T_max, int chunk_frames, int batch, void* workspace, size_t workspace_bytes,
                                void* stream);

/* hificar_ar_step with per-session conditioning (decode.py:54-83 + hifigan.py:212-220), both in caller-owned device memory addressed by
 * the table's row like ctx and c:
 *   spk_rows  (ctx_rows) int32: element `row` is the speaker of the session on that row
 *   ph        phoneme ring: frame t of the chunk of a sequence {row, frame, ...} is ph[row*ph_bstride + frame + t]; frame + valid <=
 *             ph_bstride is checked with the table
 * The step reads both when it RUNS, and up to 32 steps may be queued: write a session's speaker and its phonemes on the stream the
 * steps are given (as its features are), never from the host behind a queued step's back. */
int hificar_ar_step_cond(hificar_handle* h, const float* c, int64_t c_bstride, int64_t c_cstride, const int32_t* spk_rows,
                         const int32_t* ph, int64_t ph_bstride, const int32_t* seqs_host, int n, int chunk_frames, float* ctx,
                         int ctx_rows, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* float waveform in [-1, 1] -> 16-bit PCM on the device: y = clip(round_half_even(x *_f32 32767.f), -32768, 32767) — the product in
 * float32, as libsndfile's f2s_array computes it (lrintf(src * 32767.f)); libsndfile wraps outside [-1, 1] where this clips.
 * What the reference's sf.write(..., "PCM_16") does on the host after the device->host copy
 * (articulatory/bin/decode.py:319-324); doing it before the copy / the multi-GPU gather halves the bytes moved.
 * x, y: device pointers, n elements. */
int hificar_pcm16(const float* x, int16_t* y, size_t n, void* stream);

/* Algorithmic multiply-accumulates of one forward of B x T frames (conv + MLP MACs; bias/activation
 * excluded) — the constant SURVEY.md §8(d) defines; used by bench.py for the roofline figure. */
double hificar_macs(const hificar_handle* h, int B, int T);

/* Per-kernel timing with HIP events on the launch stream (bench.py's roofline leg; no reference
 * counterpart — the reference times whole utterances with time.time(), articulatory/bin/decode.py:302-318).
 * Between hificar_profile_begin and hificar_profile_end every kernel launch of this engine's model is bracketed
 * by two hipEvents.  hificar_profile_end synchronises the stream used, then fills up to `max_stats`
 * entries (one per distinct kernel) and writes the number of distinct kernels to *n_stats. */
typedef struct hificar_kernel_stat {
    char name[96];     /* e.g. "conv_bf16x3_kernel<4,1,4,4>" (template args as in the rocprof kernel name) */
    int64_t launches;
    double total_ms;   /* sum of hipEventElapsedTime over the launches */
    double flops;      /* algorithmic FLOPs (2 x MACs) of those launches */
    double bytes;      /* algorithmic bytes (inputs + outputs + weights read once) of those launches */
} hificar_kernel_stat;
hificar_engine* hificar_engine_of(hificar_handle* h); /* the generator's own engine (NULL for NULL) */
int hificar_profile_begin(hificar_engine* e);
int hificar_profile_end(hificar_engine* e, hificar_kernel_stat* stats, int max_stats, int* n_stats);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Training: the generator half of the reference's train step (articulatory/bin/train.py:241-440: y_ = generator(x, ar=ar) under
 * autograd, gen_loss.backward()).  The reference has no native boundary here either (PyTorch autograd through torch.nn modules);
 * these entry points stand in for  HiFiGANGenerator.forward  in training mode and the autograd graph behind it.
 * Exact-fp32 arithmetic only.
 *
 *   hificar_set_weight_device  one FOLDED parameter (name / layout as hificar_set_weight) from DEVICE memory, repacked on the
 *                              device on `stream` — the weights of a model in training live on the device and change every step
 *                              (the weight-norm fold w = v * g / ||v|| and its gradient stay with the caller's autograd).
 *                              After the first call the handle serves fp32 layer-by-layer kernels only.
 *   hificar_set_parameters_device  EVERY parameter in its RAW state_dict form from device memory in one call (two launches):
 *                              "<conv>.weight_g" + "<conv>.weight_v" for a weight-normed conv (torch.nn.utils.weight_norm, dim 0 —
 *                              hifigan.py:268-278), "<conv>.weight" for a plain one, biases, the PastFCEncoder tensors.  The fold
 *                              w = g v / ||v|| runs on the device into a master copy every pack is refreshed from.
 *   hificar_weight_norm_backward  hificar_backward's folded gradients -> gradients of those raw parameters (dg, dv of the weight
 *                              norm; the others copied): `raw_grads` holds hificar_raw_grad_floats(h) floats, one slot per entry of
 *                              the last hificar_set_parameters_device call, in its order, each slot rounded up to 4 floats.
 *   hificar_forward_train      hificar_forward that also keeps every activation the backward pass needs in `tape`
 *                              (hificar_tape_bytes(h, B, T) bytes, 256-byte aligned, caller-owned until hificar_backward returns)
 *   hificar_backward           gradients of one hificar_forward_train: dout (B, hop*T) gradient of the waveform, out the waveform
 *                              the forward returned -> `grads` (hificar_grad_floats(h) floats; parameter i of hificar_grad_count(h)
 *                              at the offset hificar_grad_info reports, in the reference's folded layout), dc (B, C, T) gradient of
 *                              the features or NULL, dar (B, ar_input) gradient of the AR context or NULL.
 *                              workspace: hificar_backward_workspace_bytes(h, B, T) bytes.
 *   hificar_forward_train_cond / hificar_backward_cond   the same pair for the conditioned generator (train.py:276 passes spk_id= / ph=
 *                              under autograd; hifigan.py:176-189, 212-220, 232-237): spk_id (B) / ph (B, T) int32 as in
 *                              hificar_forward_cond, ph_out (B, num_ph, T) the phoneme-loss head's output (use_ph_loss) or NULL; the
 *                              backward takes the SAME spk_id / ph again and dph_out (B, num_ph, T), the gradient of ph_out (NULL: ph_out
 *                              took no part in the loss).  `grads` then also holds spk_emb_mat.weight, spk_fc.{weight,bias},
 *                              ph_emb_mat.weight, ph_fc.{weight,bias} (hificar_grad_info); hificar_set_parameters_device takes them too.
 * --------------------------------------------------------------------------------------------------------------------------- */
int hificar_set_weight_device(hificar_handle* h, const char* name, const float* data, void* stream);
int hificar_set_parameters_device(hificar_handle* h, const char* const* names, const float* const* data, int n, void* stream);
int64_t hificar_raw_grad_floats(const hificar_handle* h);
int hificar_weight_norm_backward(hificar_handle* h, const float* grads, float* raw_grads, void* stream);
size_t hificar_tape_bytes(const hificar_handle* h, int B, int T);
int hificar_forward_train(hificar_handle* h, const float* c, const float* ar, float* out, int B, int T, void* workspace,
                          size_t workspace_bytes, void* tape, size_t tape_bytes, void* stream);
size_t hificar_backward_workspace_bytes(const hificar_handle* h, int B, int T);
int hificar_grad_count(hificar_handle* h);
int hificar_grad_info(hificar_handle* h, int i, char* name96, int64_t* offset, int64_t* numel);
int64_t hificar_grad_floats(hificar_handle* h);
int hificar_backward(hificar_handle* h, const float* dout, const float* out, int B, int T, const void* tape, size_t tape_bytes,
                     float* grads, float* dc, float* dar, void* workspace, size_t workspace_bytes, void* stream);
/* Data-parallel training: gradient BUCKETS.  The reference meant to wrap both networks in DistributedDataParallel (articulatory/bin/
 * train.py:1790-1801), which all-reduces buckets of gradients while the backward pass still runs.  Here a bucket is a group of parameters
 * whose gradients are complete at a known point of hificar_backward(_cond) / hificar_disc_backward:
 *   generator      bucket b < n_stages: the ResBlocks of stage n_stages - 1 - b (bucket 0 also the output conv and the phoneme head);
 *                  bucket n_stages: everything else (input conv, upsamplers, PastFCEncoder, conditioning tensors) — hificar_grad_bucket_count
 *   discriminator  one bucket per sub-discriminator (scales first, then periods) — hificar_disc_grad_bucket_count
 * hificar_raw_param_bucket(h, i) is the bucket of raw parameter i of the last hificar_set_parameters_device call.  With a callback set,
 * the backward calls fn(bucket, stream, user) on the host right after the bucket's last gradient kernel has been enqueued on `stream`
 * (the call's stream, or the sub-discriminator's side stream): the callee runs hificar_weight_norm_backward_bucket on that stream and
 * starts its collective behind it, while the backward goes on enqueueing.  The bucket variants add no cross-stream ordering. */
typedef void (*hificar_bucket_fn)(int bucket, void* stream, void* user);
int hificar_grad_bucket_count(hificar_handle* h);
int hificar_raw_param_bucket(const hificar_handle* h, int i);
int hificar_set_bucket_callback(hificar_handle* h, hificar_bucket_fn fn, void* user);
int hificar_weight_norm_backward_bucket(hificar_handle* h, const float* grads, float* raw_grads, int bucket, void* stream);
int hificar_forward_train_cond(hificar_handle* h, const float* c, const float* ar, const int32_t* spk_id, const int32_t* ph, float* out,
                               float* ph_out, int B, int T, void* workspace, size_t workspace_bytes, void* tape, size_t tape_bytes, void* stream);
int hificar_backward_cond(hificar_handle* h, const float* dout, const float* dph_out, const float* out, const int32_t* spk_id,
                          const int32_t* ph, int B, int T, const void* tape, size_t tape_bytes, float* grads, float* dc, float* dar,
                          void* workspace, size_t workspace_bytes, void* stream);

/* Parity aid: per-layer intermediates of the forwards that follow, copied into caller buffers in the reference's (B, C, L)
 * layout — what a forward hook on the reference's modules (articulatory/models/hifigan.py:221-231,
 * articulatory/layers/residual_block.py:217-221) returns.  Names:
 *   "ar_feats"                (B, ar_output)            PastFCEncoder output (pytorch_layers.py:459-460)
 *   "input_conv"              (B, channels, T)          hifigan.py:221
 *   "upsamples.<i>"           (B, C_i, L_i)             LeakyReLU + ConvTranspose1d output, hifigan.py:224
 *   "blocks.<n>.convs1.<d>"   (B, C_i, L_i)             residual_block.py:218 (runs that layer pair unfused)
 *   "blocks.<n>.x.<d>"        (B, C_i, L_i)             residual stream after dilation d: xt + x, residual_block.py:221
 *   "blocks.<n>"              (B, C_i, L_i)             block output, hifigan.py:228
 * GBlockGenerator handles (hooks on articulatory/layers/pytorch_layers.py:85-91):
 *   "ar_feats", "input_conv"  as above
 *   "resamples.<i>.conv1a"    (B, Cout_i, L_i)          first conv of conv1 (pre-activation)
 *   "resamples.<i>.res1"      (B, Cout_i, L_i)          res1(x)
 *   "resamples.<i>.mid"       (B, Cout_i, L_i)          conv1(x) + res1(x)
 *   "resamples.<i>"           (B, Cout_i, L_i)          GBlock output
 * dst: device pointer to `capacity` floats (an error is returned by the forward if it is too small); dst = NULL removes the
 * tap, name = NULL removes all.  Taps add copies and (for convs1) extra launches: not for timed runs. */
int hificar_debug_tap(hificar_handle* h, const char* name, float* dst, size_t capacity);

/* Test aid, not for production runs: from now on every conv launch of this engine (any model's: hificar_engine_of, hificar_disc_engine,
 * hificar_bigru_engine) runs tile shape (mi, wm, wn, ks, nb) instead of the one its planner would choose — mi x 32 rows per wave, wm x wn
 * MFMA waves, ks = 4: the split-K form (wm = wn = 1), nb = 2: two channel blocks per wave — wherever that launch can run the shape at all
 * (the instantiation exists for its arithmetic and K chunk, the LDS budget holds, the layers meet the register-blocked / split-K forms'
 * conditions); a launch that cannot keeps the planner's choice.  mi = 0 ends it.  The tuple must be one of the engine's 15 shapes
 * (HIFICAR_E_INVALID otherwise).  Synchronises the device and drops every cached launch plan.  Results stay correct under any shape; speed does not.
 * No reference counterpart (the reference has no tiles). */
int hificar_debug_force_tile(hificar_engine* e, int mi, int wm, int wn, int ks, int nb);

void hificar_destroy(hificar_handle* h);

const char* hificar_last_error(void);

/* Library / build identification, e.g. "hificar 0.1 gfx950". */
const char* hificar_version(void);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Discriminators of the train step: HiFiGANMultiScaleMultiPeriodDiscriminator (articulatory/models/hifigan.py:741-825; the
 * scale discriminators :503-643, the period discriminators :317-417), called at articulatory/bin/train.py:341-347 (generator
 * step: D(fake) with the gradient flowing back into the generator's waveform, D(real) without) and :421-424 (discriminator
 * step).  The reference has no native boundary here (torch.nn modules under autograd); these entry points stand in for
 * `discriminator(x)` and the autograd graph behind it.  Exact fp32.
 *
 * Layers are described explicitly (the host side derives them from discriminator_params exactly as the reference's constructors
 * do): s_* = the Conv1d stack of ONE scale discriminator (the last layer has no activation), p_* = the Conv2d (k, 1) stack of
 * ONE period discriminator (last = output_conv).  Parameter names follow the reference state_dict
 * ("msd.discriminators.0.layers.1.0.weight", "mpd.discriminators.2.convs.0.0.weight_g", ...).
 *
 *   hificar_disc_set_parameters_device   every RAW parameter from device memory (as hificar_set_parameters_device)
 *   hificar_disc_forward                 x (B, 1, T) -> every layer output of every sub-discriminator, kept in `tape`
 *                                        (hificar_disc_tape_bytes, 256-byte aligned, caller-owned); output buffer i =
 *                                        one (sub-discriminator, layer, group): [nseq][rows][pitch] floats, `channels` valid
 *                                        columns; scale discriminators: nseq = B, rows = time; period discriminators:
 *                                        nseq = B * period (sequence b * period + column), rows = T' / period.  Groups of a
 *                                        grouped conv are separate buffers (channel c of the layer = group c / channels).
 *   hificar_disc_backward                douts[i] = gradient of output buffer i (same layout) or NULL; -> grads (folded
 *                                        parameters, hificar_disc_grad_floats, offsets from hificar_disc_param_info) or NULL,
 *                                        dx (B, T) or NULL
 *   hificar_disc_weight_norm_backward    folded gradients -> raw parameter gradients (as hificar_weight_norm_backward)
 *   hificar_disc_engine                  the discriminators' engine, for hificar_profile_begin / hificar_profile_end
 * --------------------------------------------------------------------------------------------------------------------------- */
#define HIFICAR_DISC_MAX_SUBS 8
#define HIFICAR_DISC_MAX_LAYERS 12
typedef struct hificar_disc_config {
    int n_scales;                 /* scale discriminators (hifigan.py:666-738), AvgPool1d between them */
    int pool_kernel, pool_stride, pool_pad;
    int s_n_layers;
    int s_cin[HIFICAR_DISC_MAX_LAYERS], s_cout[HIFICAR_DISC_MAX_LAYERS], s_k[HIFICAR_DISC_MAX_LAYERS], s_stride[HIFICAR_DISC_MAX_LAYERS],
        s_pad[HIFICAR_DISC_MAX_LAYERS], s_groups[HIFICAR_DISC_MAX_LAYERS];
    int s_bias;
    float s_slope;
    int n_periods;                /* period discriminators (hifigan.py:451-500) */
    int periods[HIFICAR_DISC_MAX_SUBS];
    int p_n_layers;
    int p_cin[HIFICAR_DISC_MAX_LAYERS], p_cout[HIFICAR_DISC_MAX_LAYERS], p_k[HIFICAR_DISC_MAX_LAYERS], p_stride[HIFICAR_DISC_MAX_LAYERS],
        p_pad[HIFICAR_DISC_MAX_LAYERS];
    float p_slope;
} hificar_disc_config;

typedef struct hificar_disc_output {
    int sub, layer, group, n_groups;
    int period;                   /* 0: scale discriminator */
    int64_t offset_bytes;         /* inside the tape */
    int nseq, rows, pitch, channels;
} hificar_disc_output;

/* GAN criterion on the forward tapes (articulatory/losses/adversarial_loss.py:12-123, feat_match_loss.py:12-54 as combined at
 * train.py:341-362 / :421-424).  hificar_disc_loss: mode 0 = generator side (adversarial loss of the fake pass's final outputs +
 * feature matching against the real pass `tape_ref`, NULL: none): values = {adv, fm, lambda_adv * (adv + lambda_feat_match * fm)};
 * mode 1 / 2 = discriminator side, fake / real pass: values = {loss, 0, loss}.  values: 3 device floats; douts:
 * hificar_disc_dout_floats floats = d(values[2]) / d(every output buffer), consumed by hificar_disc_backward_flat. */
typedef struct hificar_gan_loss_config {
    int loss_type;                 /* 0 mse, 1 hinge */
    int average_by_discriminators; /* adversarial losses */
    int fm_average_by_layers, fm_average_by_discriminators, fm_include_final_outputs;
    float lambda_adv, lambda_feat_match;
} hificar_gan_loss_config;

typedef struct hificar_disc hificar_disc;
size_t hificar_disc_dout_floats(const hificar_disc* d, int B, int T);
int hificar_disc_loss(hificar_disc* d, const hificar_gan_loss_config* cfg, int mode, const void* tape, const void* tape_ref, int B, int T,
                      float* values3, float* douts, void* stream);
int hificar_disc_backward_flat(hificar_disc* d, const float* douts, int mode, int with_fm, int fm_include_final_outputs, int B, int T,
                               const void* tape, size_t tape_bytes, float* grads, float* dx, void* workspace, size_t workspace_bytes,
                               void* stream);
int hificar_disc_create(const hificar_disc_config* cfg, hificar_disc** out);
void hificar_disc_destroy(hificar_disc* d);
hificar_engine* hificar_disc_engine(hificar_disc* d);
int hificar_disc_param_count(const hificar_disc* d);
int hificar_disc_param_info(const hificar_disc* d, int i, char* name96, int64_t* shape4, int* ndim, int64_t* offset);
int64_t hificar_disc_grad_floats(const hificar_disc* d);
int64_t hificar_disc_raw_grad_floats(const hificar_disc* d);
int hificar_disc_set_parameters_device(hificar_disc* d, const char* const* names, const float* const* data, int n, void* stream);
int hificar_disc_weight_norm_backward(hificar_disc* d, const float* grads, float* raw_grads, void* stream);
size_t hificar_disc_tape_bytes(const hificar_disc* d, int B, int T);
/* Algorithmic multiply-accumulates of one discriminator forward over (B, 1, T) (every Conv1d / Conv2d of hifigan.py:317-825: output
 * positions x cout x cin / groups x k) — the training roofline's work unit, as hificar_macs is the generator's. */
double hificar_disc_macs(const hificar_disc* d, int B, int T);
/* gradient buckets of the discriminators (see hificar_bucket_fn above): one per sub-discriminator */
int hificar_disc_grad_bucket_count(const hificar_disc* d);
int hificar_disc_raw_param_bucket(const hificar_disc* d, int i);
int hificar_disc_bucket_folded_range(const hificar_disc* d, int bucket, int64_t* offset, int64_t* numel);
int hificar_disc_set_bucket_callback(hificar_disc* d, hificar_bucket_fn fn, void* user);
int hificar_disc_weight_norm_backward_bucket(hificar_disc* d, const float* grads, float* raw_grads, int bucket, void* stream);
/* The discriminator update backpropagates two passes (real, fake: train.py:405-437 sums their losses).  on != 0: the following
 * hificar_disc_backward* calls ADD their parameter gradients to what `grads` holds instead of overwriting it, so the second pass lands in
 * the first pass's buffer (no second buffer, no add pass).  scale_device: device scalar (or NULL) that the following
 * hificar_disc_weight_norm_backward[_bucket] calls multiply every raw gradient by while writing it — autograd's upstream gradient of the
 * scalar loss.  Both are per-handle switches; the caller resets them (0 / NULL) after the step. */
int hificar_disc_set_grad_accumulate(hificar_disc* d, int on);
int hificar_disc_set_grad_scale(hificar_disc* d, const float* scale_device);
size_t hificar_disc_backward_workspace_bytes(const hificar_disc* d, int B, int T);
int hificar_disc_output_count(const hificar_disc* d);
int hificar_disc_output_info(const hificar_disc* d, int B, int T, int i, hificar_disc_output* out);
int hificar_disc_forward(hificar_disc* d, const float* x, int B, int T, void* tape, size_t tape_bytes, void* stream);
int hificar_disc_backward(hificar_disc* d, const float* const* douts, int B, int T, const void* tape, size_t tape_bytes, float* grads,
                          float* dx, void* workspace, size_t workspace_bytes, void* stream);

/* Mel-spectrogram loss (articulatory/losses/mel_loss.py:114-166; train.py:308-311): F.l1_loss(log mel(y_hat), log mel(y)) and its
 * gradient with respect to y_hat in one call.  melmat: (num_mels, fft_size / 2 + 1) filterbank, host memory (librosa.filters.mel in the
 * reference, mel_loss.py:56-62).  window: hann (periodic, torch.hann_window), center = True, normalized = False, onesided = True.
 * log_base: 0 natural, 2 or 10. */
typedef struct hificar_mel_config {
    int fft_size, hop_size, win_length, num_mels;
    float eps;
    int log_base;
    int mode;   /* 0: mel-spectrogram loss; 1: one resolution of the multi-resolution STFT loss (melmat, num_mels, log_base unused) */
} hificar_mel_config;
typedef struct hificar_mel hificar_mel;
int hificar_mel_create(const hificar_mel_config* cfg, const float* melmat, hificar_mel** out);
void hificar_mel_destroy(hificar_mel* m);
size_t hificar_mel_workspace_bytes(const hificar_mel* m, int B, int T);
/* One resolution of MultiResolutionSTFTLoss (articulatory/losses/stft_loss.py:87-125; train.py:289-290) on a mode-1 handle: forward ->
 * values = {spectral convergence, log STFT magnitude} (2 device floats), the magnitudes stay in `workspace`; backward (same workspace):
 * dy_hat (B, T) = d(gweights[0] * sc + gweights[1] * mag) / dy_hat, gweights = 2 DEVICE floats (the upstream gradients). */
int hificar_stft_loss_forward(hificar_mel* m, const float* y_hat, const float* y, int B, int T, float* values2, void* workspace,
                              size_t workspace_bytes, void* stream);
int hificar_stft_loss_backward(hificar_mel* m, int B, int T, const float* gweights2, float* dy_hat, void* workspace, size_t workspace_bytes,
                               void* stream);
int hificar_mel_loss(hificar_mel* m, const float* y_hat, const float* y, int B, int T, float* value, float* dy_hat, void* workspace,
                     size_t workspace_bytes, void* stream);

/* Speech features of a ragged batch of waveforms, on the device (forward only; exact fp32).
 *   HIFICAR_FEAT_MFCC    librosa 0.8.1's feature.mfcc as egs/ema/voc1/local/predict_ema.py:32-33 calls it: P = |STFT|^2, mel = fb P,
 *                        dB = 10 log10(max(amin, mel)), dB = max(dB, max over the utterance's own frames and bands - top_db) (top_db < 0: no
 *                        clamp), orthonormal DCT-II over the bands, the first n_mfcc coefficients.  No z-score: hificar_*_forward_lowrate's.
 *   HIFICAR_FEAT_LOGMEL  articulatory/bin/preprocess.py:58-82: log_b(max(amin, fb |STFT|)), log_base 0 (natural), 2 or 10; amin is its eps.
 * STFT: center = True with reflect padding of fft_size / 2 at the utterance's own two ends, periodic Hann of win_length centred in the frame,
 * 1 + L / hop_size frames for L samples.  melmat: (num_mels, fft_size / 2 + 1) filterbank, host memory (librosa.filters.mel in the
 * reference).  hificar_feat_create touches no device (it checks the configuration and builds host tables); the first hificar_feat_forward
 * whose arguments pass every check sets the device state up.
 *
 * hificar_feat_forward: wav (B, Lmax) device floats; lengths: device int32[B] sample counts, or NULL (every utterance has Lmax); lengths_host:
 * the same numbers in host memory, or NULL — given, every entry is checked (fft_size / 2 < l <= Lmax) before anything is enqueued; not
 * given, the kernels clamp a length into 0 .. Lmax and give an utterance of fft_size / 2 samples or fewer no frames.  out: (B, C, Tmax), C =
 * n_mfcc | num_mels, Tmax = hificar_feat_frames(h, Lmax), exactly zero from an utterance's own frame count on; frames_out: device int32[B]
 * (those counts) or NULL.  Samples at or past a length are never read, and an utterance's result is bit for bit that of running it alone
 * (split-K off, fixed-order reductions, no atomics).  workspace: 256-byte aligned, hificar_feat_workspace_bytes(h, B, Lmax) bytes (0: the
 * shape is refused).  Lmax <= fft_size / 2: HIFICAR_E_INVALID. */
#define HIFICAR_FEAT_LOGMEL 0
#define HIFICAR_FEAT_MFCC 1
#define HIFICAR_FEAT_MAX_MELS 128
typedef struct hificar_feat_config {
    int kind;       /* HIFICAR_FEAT_LOGMEL | HIFICAR_FEAT_MFCC */
    int fft_size;   /* a multiple of 32, 32 .. 8192 */
    int hop_size, win_length;
    int num_mels;   /* 1 .. HIFICAR_FEAT_MAX_MELS */
    int n_mfcc;     /* MFCC: 1 .. num_mels */
    float amin;     /* MFCC: power_to_db's amin (1e-10); log-mel: eps */
    float top_db;   /* MFCC: power_to_db's top_db (80); negative: none */
    int log_base;   /* log-mel: 0 natural, 2 or 10 */
} hificar_feat_config;
typedef struct hificar_feat hificar_feat;
int hificar_feat_create(const hificar_feat_config* cfg, const float* melmat, hificar_feat** out);
void hificar_feat_destroy(hificar_feat* h);
hificar_engine* hificar_feat_engine(hificar_feat* h);     /* for hificar_profile_begin / hificar_profile_end */
int hificar_feat_frames(const hificar_feat* h, int L);   /* 1 + L / hop_size; 0 for L <= fft_size / 2 */
size_t hificar_feat_workspace_bytes(const hificar_feat* h, int B, int Lmax);
int hificar_feat_forward(hificar_feat* h, const float* wav, const int32_t* lengths, const int32_t* lengths_host, float* out, int32_t* frames_out,
                         int B, int Lmax, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Articulatory inversion: the BiGRU speech-to-EMA model (articulatory/models/pytorch_models.py:22-123) in eval mode — two bidirectional
 * GRU layers (torch.nn.GRU, gate order r, z, n, h0 = 0), Linear(2H, 128), BatchNorm1d(128) on running statistics, Linear(128, out) and an
 * optional tanh.  The reference has no native boundary here either (torch.nn modules; driven by model.inference, articulatory/bin/decode.py:338-350).
 * Exact fp32.  Errors as everywhere: a negative HIFICAR_E_* code and hificar_last_error().
 * --------------------------------------------------------------------------------------------------------------------------- */
#define HIFICAR_BIGRU_MAX_IN 4096
#define HIFICAR_BIGRU_MAX_HIDDEN 256
#define HIFICAR_BIGRU_MAX_OUT 32

/* Mirrors the keyword arguments of BiGRU.__init__ (pytorch_models.py:23-25) that affect eval-mode inference; use_ar and use_spk_emb
 * models are not built (the binding refuses them). */
typedef struct hificar_bigru_config {
    int32_t in_channels;  /* 1 .. HIFICAR_BIGRU_MAX_IN */
    int32_t hidden_size;  /* a multiple of 64, at most HIFICAR_BIGRU_MAX_HIDDEN: one workgroup holds one direction's W_hh */
    int32_t out_channels; /* 1 .. HIFICAR_BIGRU_MAX_OUT */
    int32_t use_tanh;     /* fc2 = Sequential(Linear, Tanh): its tensors are then named "fc2.0.*" (pytorch_models.py:34-37) */
} hificar_bigru_config;

typedef struct hificar_bigru hificar_bigru;

/* BiGRU.__init__ (pytorch_models.py:23-43): an empty model for these hyper-parameters on the current HIP device. */
int hificar_bigru_create(const hificar_bigru_config* cfg, hificar_bigru** out);

/* load_state_dict (articulatory/utils/utils.py:340-342), one tensor at a time by its reference state_dict name: "gru1.weight_ih_l0"
 * (3H, in_channels), "gru2.weight_ih_l0" (3H, 2H), "gru<l>.weight_hh_l0" (3H, H), "gru<l>.bias_ih_l0" / "gru<l>.bias_hh_l0" (3H), each also
 * with the suffix "_reverse"; "fc1.0.weight" (128, 2H), "fc1.0.bias"; "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var" (128);
 * "fc2.weight" (out, 128), "fc2.bias" — "fc2.0.*" with use_tanh.  data: HOST pointer to contiguous fp32; the caller keeps ownership. */
int hificar_bigru_set_weight(hificar_bigru* h, const char* name, const float* data, const int64_t* shape, int ndim);

/* model.eval().to(device) (decode.py:276-277): checks that every tensor arrived, folds the batch norm into fc1, repacks, uploads.
 * Synchronises the device once. */
int hificar_bigru_finalize(hificar_bigru* h);

/* Bytes of device scratch hificar_bigru_forward needs for B sequences of T frames: the pre-gate buffer (B T 6H floats, shared by the two
 * GRU layers) and one row buffer (B T max(in_channels, 2H) floats).  (torch's caching allocator does this implicitly in the reference.) */
size_t hificar_bigru_workspace_bytes(const hificar_bigru* h, int B, int T);

/* BiGRU.forward in eval mode (pytorch_models.py:45-72): x (B, in_channels, T) device fp32 -> out (B, out_channels, T) device fp32.
 * lengths: DEVICE pointer to B int32 frame counts (0 <= lengths[b] <= T) or NULL (all T): sequence b is computed exactly as if it were alone
 * with lengths[b] frames — its reverse direction starts at its own last frame — and out[b, :, lengths[b]:] is written as zeros.  The
 * reference has no such batches: this is its per-utterance loop (decode.py:292-351) run B utterances at a time.  lengths_host: optional HOST
 * copy of the same values (NULL = unknown to the host), checked against T before anything is enqueued.  workspace: 256-byte aligned,
 * hificar_bigru_workspace_bytes(h, B, T) bytes.  Stream rules as in the conventions at the top. */
int hificar_bigru_forward(hificar_bigru* h, const float* x, const int32_t* lengths, const int32_t* lengths_host, float* out, int B, int T,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- The low-rate front end: the step between "features from the speech model" and the model's forward in the reference's speech-to-EMA
 * driver (egs/ema/voc1/local/predict_ema.py:83-101), on the device and without a stretched or normalised copy of the input.
 *   factor   1 .. HIFICAR_LOWRATE_MAX_FACTOR.  A sequence of l low-rate frames becomes factor * l frames by the rule of
 *            F.interpolate(size=factor * l, mode='linear', align_corners=False) (predict_ema.py:86-90; the reference uses 4, or 2 for its hprc
 *            models): src = max(0, (t + 0.5) / factor - 0.5), i0 = floor(src), i1 = min(i0 + 1, l - 1), lam = src - i0,
 *            y[t] = (1 - lam) x[i0] + lam x[i1].  Every sequence of a batch clamps at its OWN first and last frame.  l = 0: no frames; l = 1: the
 *            frame factor times; factor = 1: the identity.
 *   zscore   != 0: per utterance (x - mean) / std, mean and std (population) over all in_channels * l elements of its valid frames, as
 *            scipy.stats.zscore(feat, axis=None) (predict_ema.py:32-35): two passes in double, a fixed summation order.  std = 0 gives what
 *            IEEE division gives (NaN), as scipy does.  With both options the normalisation comes first (either order is the same function).
 * An utterance's result does not depend on what it is batched with, bit for bit; padded input frames are never read, and what the workspace
 * holds on entry does not matter. ---- */
#define HIFICAR_LOWRATE_MAX_FACTOR 16

/* Bytes of device scratch hificar_bigru_forward_lowrate needs for B sequences of Tl low-rate frames: the pre-gate buffer at the model's rate
 * (B factor Tl 6H floats), layer 1's pre-gates at the low rate (B Tl 6H floats; none at factor 1), one row buffer of
 * max(Tl in_channels, factor Tl 2H) floats per sequence, and the per-utterance statistics and frame counts.  0: arguments out of range. */
size_t hificar_bigru_workspace_bytes_lowrate(const hificar_bigru* h, int B, int Tl, int factor);

/* predict_ema.py:83-101 for the BiGRU: x (B, in_channels, Tl) device fp32, lengths LOW-RATE frame counts (device; NULL: all Tl; lengths_host as
 * in hificar_bigru_forward, checked against Tl) -> out (B, out_channels, factor * Tl), zero past factor * lengths[b].  Layer 1's input projection
 * runs over the B Tl low-rate rows and its pre-gates are interpolated (interp(X) W + b = interp(X W + b): the two weights sum to one); from
 * the first sweep on the launches are hificar_bigru_forward's.  factor = 1 and zscore = 0 IS hificar_bigru_forward: the same launches, the same
 * bits.  Every argument is checked on the host before anything is enqueued; HIFICAR_E_STATE before hificar_bigru_finalize.  workspace: 256-byte
 * aligned, hificar_bigru_workspace_bytes_lowrate(h, B, Tl, factor) bytes. */
int hificar_bigru_forward_lowrate(hificar_bigru* h, const float* x, const int32_t* lengths, const int32_t* lengths_host, float* out, int B, int Tl,
                                  int factor, int zscore, void* workspace, size_t workspace_bytes, void* stream);

/* The model's engine, for hificar_profile_begin / hificar_profile_end (the reference times whole utterances, decode.py:302-318). */
hificar_engine* hificar_bigru_engine(hificar_bigru* h);

/* del model */
void hificar_bigru_destroy(hificar_bigru* h);

/* ---- BiGRU training: the reference's step for dataset_mode art / a2m / m2a (articulatory/bin/train.py:241-383), the model in train() mode:
 * Dropout(p) behind each GRU layer and fc1, BatchNorm1d on batch statistics.  Exact fp32, deterministic (fixed-order reductions).
 * hificar_bigru_forward_train takes equal-length batches (the reference's CollaterMelArt cuts equal windows);
 * hificar_bigru_forward_train_ragged takes whole utterances of unequal lengths (this library's definition: the reference never masks).
 * All of these may be called after hificar_bigru_finalize; the first one builds the training state.
 * Training on low-rate inputs: hificar_bigru_forward_train_lowrate / hificar_bigru_backward_lowrate, behind hificar_bigru_backward.
 * Not built: multi-GPU BiGRU training, packed (padding-free) GEMMs for ragged batches (the Transformer has them:
 * hificar_xfmr_forward_train_packed), the gradient through the z-score's statistics, use_ar, use_spk_emb. ---- */

/* Every float tensor of the state_dict (reference names and layouts, bn.running_mean / bn.running_var included; n = all of them, each
 * once) from DEVICE memory.  The handle copies them and rebuilds every derived form on the device, on `stream`: the GEMM packs, W_hh and
 * its transpose in the recurrent kernels' orders, and the eval-mode fold of the batch norm into fc1 — hificar_bigru_forward sees the
 * new weights too.  Call it after every optimizer step (and before the first hificar_bigru_forward_train).  Every name is checked before any
 * byte is copied: a list that is refused (HIFICAR_E_INVALID: another count, a null entry, an unknown or a repeated name) leaves the handle
 * exactly as it was. */
int hificar_bigru_set_parameters_device(hificar_bigru* h, const char* const* names, const float* const* data, int n, void* stream);

/* The gradient buffer: hificar_bigru_grad_floats(h) floats; tensor i of hificar_bigru_grad_count(h) has the reference's state_dict name
 * (name96: at least 96 bytes) and layout, at `offset` floats, `numel` long.  Same contract as hificar_grad_info. */
int hificar_bigru_grad_count(hificar_bigru* h);
int hificar_bigru_grad_info(hificar_bigru* h, int i, char* name96, int64_t* offset, int64_t* numel);
int64_t hificar_bigru_grad_floats(hificar_bigru* h);

/* Bytes of the tape (what a training forward keeps for its backward pass: the input rows, both layers' hidden states and per-step gate
 * values r, z, n, W_hn h + b_hn, the raw fc1 rows, the batch statistics, the output, a ragged forward's lengths (in rows a dense tape
 * leaves unused: both forms take the same size) and their sum; dropout masks are regenerated, not stored) and of
 * the scratch shared by hificar_bigru_forward_train and hificar_bigru_backward. */
size_t hificar_bigru_tape_bytes(const hificar_bigru* h, int B, int T);
size_t hificar_bigru_train_workspace_bytes(hificar_bigru* h, int B, int T);

/* BiGRU.forward in train() mode: x (B, in_channels, T) -> out (B, out_channels, T), device fp32.  Dropout: element e of site s (0: gru1's
 * output, 1: gru2's, 2: fc1's; e = the element's index in the (B, T, C) tensor) is kept when u(seed, offset, s, e) >= dropout_p and scaled
 * by 1 / (1 - dropout_p); u is a counter-based generator (numpy restatement: articulatory_amd.utils.synth.bigru_dropout_mask), `offset`
 * the caller's count of training forwards.  dropout_p = 0 is the identity.  bn_batch_stats: 2 x 128 device floats, this batch's
 * per-channel mean and BIASED variance (the caller updates running_mean / running_var as torch.nn.BatchNorm1d does).  B * T >= 2.
 * tape / workspace: 256-byte aligned device memory of at least the sizes above; the tape is the caller's until hificar_bigru_backward ran.
 * tape = NULL (tape_bytes ignored): the same arithmetic and outputs without a tape, for a training-mode forward that no backward follows. */
int hificar_bigru_forward_train(hificar_bigru* h, const float* x, float* out, float* bn_batch_stats, int B, int T, float dropout_p, uint64_t seed,
                                uint64_t offset, void* tape, size_t tape_bytes, void* workspace, size_t workspace_bytes, void* stream);

/* The same step on a ragged batch of whole utterances: sequence b has lengths[b] frames (0 .. T; M = their sum >= 2) of x (B, in_channels, T);
 * what x holds past them is never used (NaN included).
 *   GRU layers   sequence b is swept over its own lengths[b] frames; the reverse direction starts at its own last frame (as
 *                hificar_bigru_forward does in eval mode)
 *   dropout      element e is the index in the PADDED (B, T, C) tensor, as above: the masks depend on T, not only on the lengths
 *   batch norm   mean and biased variance over the M valid rows; bn_batch_stats as above (the caller's running variance takes M / (M - 1))
 *   out          out[b, :, lengths[b]:] is exactly zero
 * lengths: device int32[B], B <= 32768.  lengths_host: the same values on the host, required: each is checked against 0 .. T and their sum against >= 2
 * before anything is enqueued (HIFICAR_E_INVALID otherwise).  The tape records the lengths and M, so hificar_bigru_backward takes no new
 * argument and cannot be run with other lengths than its forward: on such a tape it ignores dout on padded frames, whatever it holds, writes
 * dx = 0 there, and every weight and bias gradient sums valid frames only.  With all lengths = T every result is bitwise that of
 * hificar_bigru_forward_train.  Deterministic (no atomics).  tape = NULL: the forward-only form, as above.
 * The GEMMs still run over all B T rows (zeros in the padded rows mask them): padding costs time, not correctness. */
int hificar_bigru_forward_train_ragged(hificar_bigru* h, const float* x, const int32_t* lengths, const int32_t* lengths_host, float* out,
                                       float* bn_batch_stats, int B, int T, float dropout_p, uint64_t seed, uint64_t offset, void* tape,
                                       size_t tape_bytes, void* workspace, size_t workspace_bytes, void* stream);

/* dout (B, out_channels, T) -> grads (hificar_bigru_grad_floats floats: written, not accumulated) and, with dx non-NULL, the input's
 * gradient (B, in_channels, T).  The weights must be those of the forward that filled the tape.  A tape of
 * hificar_bigru_forward_train_ragged: see there. */
int hificar_bigru_backward(hificar_bigru* h, const float* dout, int B, int T, const void* tape, size_t tape_bytes, float* grads, float* dx,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ---- Training on low-rate inputs: the step above on x (B, in_channels, Tl) at 1 / factor of the model's rate (and / or z-scored per utterance),
 * as the low-rate front end defines them (factor, zscore: see HIFICAR_LOWRATE_MAX_FACTOR), T = factor * Tl.  The results are those of
 * hificar_bigru_forward_train[_ragged] on the stretched input, to rounding: interp(X) W + b = interp(X W + b) also holds under the chain rule
 * (A: the interpolation matrix; dW_ih = (A^T dGX)^T X_low, db_ih = column sums of A^T dGX, dX_low = (A^T dGX) W_ih), so layer 1's projection, weight
 * gradient and data gradient run over the B Tl low-rate rows and no stretched copy of the input exists, on the tape or anywhere else.
 * Tape: the header (it records factor, Tl and zscore), the input block [B Tl (+ slack)][in_channels rounded up to 32] of LOW-RATE rows, and behind
 * it the tape of hificar_bigru_tape_bytes(h, B, factor * Tl) unchanged; the 16 bytes of statistics per utterance of a z-scored forward lie in
 * slack rows of that tape, as the lengths do (so B <= 8192 with zscore).  Workspace: that of hificar_bigru_train_workspace_bytes(h, B, factor * Tl)
 * (the block a tape-less forward keeps its rows in holds the low-rate input block too) and a [B Tl][6H] buffer (the low-rate pre-gates; backwards
 * the adjoint interpolation's output).  At factor 1 both sizes are those of the existing functions.  0: arguments out of range. ---- */
size_t hificar_bigru_tape_bytes_lowrate(const hificar_bigru* h, int B, int Tl, int factor);
size_t hificar_bigru_train_workspace_bytes_lowrate(hificar_bigru* h, int B, int Tl, int factor);

/* lengths = NULL (with lengths_host = NULL): the dense form.  Otherwise both are required, LOW-RATE frame counts in 0 .. Tl: sequence b has
 * factor * lengths[b] frames at the model's rate and is interpolated by its own length (clamped at its own last frame); the step is
 * hificar_bigru_forward_train_ragged's on the stretched batch: the dropout masks are those of the (B, T, C) tensors, the batch statistics run over
 * M = factor * sum(lengths) >= 2 rows, out (B, out_channels, factor * Tl) is zero past factor * lengths[b]; padded low-rate frames of x are never
 * read.  zscore != 0: every utterance is normalised by its own statistics first, which the backward pass takes as constants.
 * tape = NULL: the forward-only form.  Every argument is checked on the host before anything is enqueued, the handle's state last.
 * factor = 1 and zscore = 0 IS hificar_bigru_forward_train[_ragged]: the same launches, the same bits, the same tape. */
int hificar_bigru_forward_train_lowrate(hificar_bigru* h, const float* x, const int32_t* lengths, const int32_t* lengths_host, float* out,
                                        float* bn_batch_stats, int B, int Tl, int factor, int zscore, float dropout_p, uint64_t seed, uint64_t offset,
                                        void* tape, size_t tape_bytes, void* workspace, size_t workspace_bytes, void* stream);

/* The backward pass on a tape of hificar_bigru_forward_train_lowrate: dout (B, out_channels, factor * Tl) -> grads as hificar_bigru_backward
 * writes them and, with dx non-NULL, the input's gradient at the LOW rate (B, in_channels, Tl), exactly zero on padded low-rate frames.
 * A separate entry point: the tape's header lives in device memory, so hificar_bigru_backward could learn the layout of the tape it is handed
 * only through a synchronising copy.  B, Tl, factor and zscore must be the forward's (as B and T must be for hificar_bigru_backward; a tape is
 * not portable between factors).  dx with zscore != 0 is HIFICAR_E_INVALID: the statistics' own derivative is not built.
 * factor = 1 and zscore = 0 IS hificar_bigru_backward.  The adjoint interpolation (bigru_interp_gates_adj_kernel) is a gather with a fixed
 * summation order: deterministic, and a sequence's dx does not depend on what it is batched with. */
int hificar_bigru_backward_lowrate(hificar_bigru* h, const float* dout, int B, int Tl, int factor, int zscore, const void* tape, size_t tape_bytes,
                                   float* grads, float* dx, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Feature-to-feature mapping: the Transformer encoder (articulatory/models/transformer.py:21-105; layers articulatory/layers/pytorch_layers.py:94-423)
 * in eval mode — three ResBlocks (Conv1d k = 3 + BatchNorm1d on running statistics, ReLU), Linear, `elayers` post-LayerNorm encoder layers
 * (8-head self-attention with learned relative positions up to distance 100, a 3072-wide ReLU feed-forward), Linear.  nhead = 8,
 * dim_feedforward = 3072 and relative_positional_distance = 100 are the reference constructor's constants.  The attention is computed in its
 * banded form: a sequence of more than 100 frames has every logit with |k - q| >= 100 lowered by 1e8 in the reference (weight exactly 0 in
 * fp32), so only keys with |k - q| <= 99 are visited.  Training: the block behind hificar_xfmr_destroy.  Not built: extra_art, num_ph
 * (the binding refuses them).
 * Exact fp32 by default.  Opt-in bf16x3 (hificar_xfmr_set_precision, inference only): every GEMM — the ResBlock convs and residual_path,
 * w_raw_in, q | k | v, w_o, linear1, linear2, w_out — runs in the conv engine's bf16x3 kernels (x w ~ hi hi + hi lo + lo hi on bf16 MFMAs, fp32
 * accumulation); the attention, LayerNorm, bias and residual additions and the residual stream stay fp32.  The training step has the same
 * opt-in for its forward GEMMs and data gradients (hificar_xfmr_set_train_precision, below).
 * Opt-in bf16x3a (HIFICAR_PREC_BF16X3A, inference only): bf16x3, and the attention's three products (Q K^T, Q E^T, P V) as hi hi + hi lo + lo hi
 * on v_mfma_f32_16x16x32_bf16 as well, in a kernel of its own (xfmr_attn16_kernel) that reads q | k | v as split rows — the q | k | v GEMM
 * writes nothing else — and position tables split once at finalize; softmax, LayerNorm, additions and the residual stream stay fp32.  Such a
 * handle is a bf16x3 handle everywhere else: the same workspace, the same refusals.
 * Not built: bf16 MFMAs in the training attention's key-tiled backward (dK, dV, the table gradient), bf16x3 weight-gradient kernels of the
 * k = 3 convs.
 * Errors as everywhere: a negative HIFICAR_E_* code and hificar_last_error().
 * --------------------------------------------------------------------------------------------------------------------------- */
#define HIFICAR_XFMR_MAX_IN 4096
#define HIFICAR_XFMR_MAX_OUT 1024
#define HIFICAR_XFMR_MAX_HIDDEN 1024
#define HIFICAR_XFMR_MAX_LAYERS 24

/* Mirrors the keyword arguments of Transformer.__init__ (transformer.py:22-24) that shape eval-mode inference. */
typedef struct hificar_xfmr_config {
    int32_t in_channels;  /* 1 .. HIFICAR_XFMR_MAX_IN */
    int32_t out_channels; /* 1 .. HIFICAR_XFMR_MAX_OUT */
    int32_t elayers;      /* 1 .. HIFICAR_XFMR_MAX_LAYERS */
    int32_t hidden_dim;   /* a multiple of 128, at most HIFICAR_XFMR_MAX_HIDDEN: head size hidden_dim / 8 = 16 .. 128 in steps of 16 */
} hificar_xfmr_config;

typedef struct hificar_xfmr hificar_xfmr;

/* Transformer.__init__: an empty model for these hyper-parameters.  Touches no device. */
int hificar_xfmr_create(const hificar_xfmr_config* cfg, hificar_xfmr** out);

/* load_state_dict, one tensor at a time by its reference state_dict name: "conv_blocks.<i>.conv1.weight" (F, C or F, 3), ".conv1.bias",
 * ".bn1.weight" / ".bias" / ".running_mean" / ".running_var" (F), the same for conv2 / bn2, and for block 0 of a model with in_channels != F
 * "conv_blocks.0.residual_path.weight" (F, C, 1), ".bias", "conv_blocks.0.res_norm.*"; "w_raw_in.weight" (F, F), ".bias";
 * "transformer.layers.<l>.self_attn.w_q" / "w_k" / "w_v" (8, F, d), ".w_o" (8, d, F), ".relative_positional.embeddings" (8, 199, d, 1),
 * ".linear1.weight" (3072, F), ".linear2.weight" (F, 3072), their biases, ".norm1" / ".norm2" ".weight" / ".bias" (F); "w_out.weight" (out, F),
 * "w_out.bias".  F = hidden_dim, d = F / 8.  data: HOST pointer to contiguous fp32; the caller keeps ownership. */
int hificar_xfmr_set_weight(hificar_xfmr* h, const char* name, const float* data, const int64_t* shape, int ndim);

/* The arithmetic of the handle's GEMMs: HIFICAR_PREC_F32 (the default), HIFICAR_PREC_BF16X3, or HIFICAR_PREC_BF16X3A (bf16x3 with the
 * attention on bf16 MFMAs too; whatever is said of a bf16x3 handle below holds for it).  Legal between hificar_xfmr_create and
 * hificar_xfmr_finalize only (HIFICAR_E_STATE afterwards): finalize packs the weight fragments of the chosen arithmetic alone and drops the host
 * tensors.  An unknown value: HIFICAR_E_INVALID.  Touches no device.  A bf16x3 handle serves hificar_xfmr_forward; every training entry point
 * and hificar_xfmr_set_parameters_device refuse it with HIFICAR_E_STATE (bf16x3 training is an f32 handle's
 * hificar_xfmr_set_train_precision), and so does the debug
 * tap "conv_blocks" with HIFICAR_E_INVALID (those rows exist as split bf16 rows only).  As in exact fp32, split-K is off: a sequence's result
 * does not depend on what it is batched with. */
int hificar_xfmr_set_precision(hificar_xfmr* h, int precision);

/* model.eval().to(device): checks that every tensor arrived, folds the batch norms into their convs (in double), repacks w_q / w_k / w_v into
 * one GEMM and w_o into another, uploads.  Synchronises the device once. */
int hificar_xfmr_finalize(hificar_xfmr* h);

/* Bytes of device scratch hificar_xfmr_forward needs for B sequences of T frames: the input rows, three row buffers of hidden_dim floats (five
 * on a bf16x3 handle: the layer input and norm1's output exist as fp32 rows and as split rows at once) and one of 3072 floats per frame (B T
 * rounded up to 256 rows).  Answers for the handle's arithmetic as it stands: ask after hificar_xfmr_set_precision. */
size_t hificar_xfmr_workspace_bytes(const hificar_xfmr* h, int B, int T);

/* Transformer.forward in eval mode (transformer.py:55-77): x (B, in_channels, T) device fp32 -> out (B, out_channels, T) device fp32.
 * lengths: DEVICE pointer to B int32 frame counts (0 <= lengths[b] <= T) or NULL (all T): sequence b is computed exactly as if it were alone
 * with lengths[b] frames — the convs see zero padding at its own end, its keys stop at its length — bit for bit, and out[b, :, lengths[b]:]
 * is written as zeros; what x holds past a length is never read.  The reference has no such batches: this is its per-utterance loop
 * (articulatory/bin/decode.py:292-351) run B utterances at a time.  lengths_host: optional HOST copy of the same values, checked against T before
 * anything is enqueued.  workspace: 256-byte aligned, hificar_xfmr_workspace_bytes(h, B, T) bytes; what it holds on entry does not matter.
 * B T 3072 < 2^31.  Stream rules as in the conventions at the top. */
int hificar_xfmr_forward(hificar_xfmr* h, const float* x, const int32_t* lengths, const int32_t* lengths_host, float* out, int B, int T,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Bytes of device scratch hificar_xfmr_forward_lowrate needs: hificar_xfmr_workspace_bytes(h, B, factor * Tl) and the per-utterance statistics and
 * frame counts.  0: arguments out of range. */
size_t hificar_xfmr_workspace_bytes_lowrate(const hificar_xfmr* h, int B, int Tl, int factor);

/* predict_ema.py:83-101 for the Transformer (the low-rate front end described at hificar_bigru_forward_lowrate: the same factor, zscore, lengths
 * and guarantees): x (B, in_channels, Tl) -> out (B, out_channels, factor * Tl), zero past factor * lengths[b].  The input rows are formed at the
 * model's rate from the low-rate input in one kernel (on a bf16x3 / bf16x3a handle as split rows, with the fp32 residual copy when in_channels ==
 * hidden_dim); every launch behind them is hificar_xfmr_forward's.  factor = 1 and zscore = 0 IS hificar_xfmr_forward.  B factor Tl 3072 < 2^31. */
int hificar_xfmr_forward_lowrate(hificar_xfmr* h, const float* x, const int32_t* lengths, const int32_t* lengths_host, float* out, int B, int Tl,
                                 int factor, int zscore, void* workspace, size_t workspace_bytes, void* stream);

/* Test aid: the following forwards also copy the named intermediate, as rows (B, T, hidden_dim), into dst (device, `capacity` floats).
 * Names: "conv_blocks", "w_raw_in", "layers.<l>.norm1" (the attention sub-block's output), "layers.<l>" (the layer's output).
 * hificar_xfmr_forward_train serves three more, the outputs of its ReLUs (which side of each the device took): "conv_blocks.<n>.relu1",
 * "conv_blocks.<n>.relu2" (rows of hidden_dim) and "layers.<l>.hidden" (rows of 3072, before the dropout); hificar_xfmr_forward_train_ragged
 * serves the same names, the rows of padded frames as zeros.
 * name = NULL forgets every tap, dst = NULL that one. */
int hificar_xfmr_debug_tap(hificar_xfmr* h, const char* name, float* dst, size_t capacity);

/* The model's engine, for hificar_profile_begin / hificar_profile_end. */
hificar_engine* hificar_xfmr_engine(hificar_xfmr* h);

/* del model */
void hificar_xfmr_destroy(hificar_xfmr* h);

/* ---- Transformer training: the reference's step for dataset_mode art / a2m / m2a (articulatory/bin/train.py:241-383), the model in train()
 * mode: BatchNorm1d on batch statistics in the three ResBlocks, Dropout(p) on the attention probabilities, behind the attention and feed-forward
 * sub-blocks and on the feed-forward's hidden rows.  Exact fp32, deterministic: every reduction is summed in a fixed order, no floating-point
 * atomics.  hificar_xfmr_forward_train takes equal-length batches (the reference's CollaterMelArt cuts equal windows);
 * hificar_xfmr_forward_train_ragged takes whole utterances of unequal lengths (this library's definition: the reference never masks), and
 * hificar_xfmr_forward_train_packed computes the same step without GEMM rows for the padding.
 * All of these may be called after hificar_xfmr_finalize; the first one builds the training state.
 * The forward GEMMs and data gradients have an opt-in bf16x3 arithmetic (hificar_xfmr_set_train_precision, below).
 * The one-tap weight gradients have one too (HIFICAR_PREC_BF16X3W), and so have the attention's query-tiled kernels (HIFICAR_PREC_BF16X3WA)
 * the weight gradients of the wide k = 3 convs (HIFICAR_PREC_BF16X3WAC) and the attention's key-tiled backward (HIFICAR_PREC_BF16X3WACK).
 * Not built: a smaller tape per frame, a k = 3 weight-gradient kernel that forms the three taps from one staged chunk, a key-major or pre-split copy of the dS / Pd bands, extra_art, num_ph, multi-GPU training of this model. ---- */

/* The arithmetic of the training step's GEMMs: HIFICAR_PREC_F32 (the default: the step above, bit for bit), HIFICAR_PREC_BF16X3,
 * HIFICAR_PREC_BF16X3W, HIFICAR_PREC_BF16X3WA, HIFICAR_PREC_BF16X3WAC or HIFICAR_PREC_BF16X3WACK.
 * bf16x3: every forward GEMM of hificar_xfmr_forward_train / _ragged / _packed (the six ResBlock convs and residual_path, w_raw_in,
 * q | k | v, w_o, linear1, linear2, w_out) and every data gradient of the same layers runs as x w ~ hi hi + hi lo + lo hi on bf16 MFMAs with
 * fp32 accumulation, in the conv engine's bf16x3 kernels (hi = bf16(x), lo = bf16(x - hi), round to nearest even; split-K off: one
 * accumulation order whatever the batch).  Weight and bias gradients stay exact fp32 on the tape's fp32 rows; so do the attention forward
 * and backward, softmax, LayerNorm and BatchNorm, dropout (the same masks), bias and residual additions, and the tape's contents and layout
 * (hificar_xfmr_tape_bytes* do not change).  hificar_xfmr_forward stays exact fp32.  hificar_xfmr_set_parameters_device then also builds the
 * bf16 fragments of every forward and data-gradient layer on the device, and the training workspace grows by one buffer of split rows
 * (3072 columns): ask hificar_xfmr_train_workspace_bytes* after this call.
 * bf16x3w: the bf16x3 step, bit for bit in its forward, data gradients, attention, norms, dropout masks, tape and eval forward, and in
 * addition the weight gradient of every one-tap layer at least 128 output channels and 128 input columns wide (w_raw_in, q | k | v, w_o,
 * linear1, linear2 at the default size) as dW = G^T A ~ hi^T hi + hi^T lo + lo^T hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation, on
 * operands split the same way (hi = bf16(x), lo = bf16(x - hi)) into groups of 8 rows per column; the bias gradient of such a layer is the
 * fp32 sum of hi + lo over the rows.  Deterministic (fixed summation order, no atomics).  Every other weight and bias gradient — the k = 3
 * ResBlock convs, residual_path, w_out, anything narrower than 128 — stays on the exact fp32 kernels.  The workspace grows by two more
 * buffers (the split G and A rows, 3072 columns each) behind the bf16x3 one.  bf16x3 <-> bf16x3w rebuilds nothing.
 * bf16x3wa: the bf16x3w step, bit for bit in every launch outside the attention, with the attention's two query-tiled kernels on
 * v_mfma_f32_16x16x32_bf16 (hi hi + hi lo + lo hi, fp32 accumulation, operands split as above).  Forward (dense, ragged, packed): S^T = K Q^T,
 * the positional product E Q^T and O^T += V^T Pd^T; softmax statistics, the online rescale, L = m + log l and the division by l stay fp32, the
 * dropout factor (the same element index, so the same masks) is applied to the kept probabilities before P V.  Backward: S recomputed with the
 * forward's own MFMA sequence, dPd^T = V dO^T and both parts of dQ (K^T dS^T, E^T dS^T) in the same form; Delta, the exponential and dS stay
 * fp32, and dS and Pd go to the same banded fp32 buffers, which the key-tiled kernels (dK, dV, the table gradient: exact fp32, unchanged)
 * read.  The tape keeps fp32 q | k | v, O and lse rows (its size does not change): a fetched key block is split on its way into LDS.  The
 * position tables are split on the device behind every parameter hand-over (8 x 208 x d bf16, twice, per layer; handle state, no workspace).
 * bf16x3w <-> bf16x3wa rebuilds no weight pack (towards bf16x3wa the tables are split).
 * bf16x3wac: the bf16x3wa step, bit for bit in every launch but the weight (and bias) gradients of the k = 3 convs that have at least 128 output
 * channels, input rows of 128 .. 1024 columns (cin_pad) and one phase: conv_blocks.{1,2}.conv1 and conv_blocks.{0,1,2}.conv2 at any hidden size,
 * conv_blocks.0.conv1 where in_channels pads to 128 .. 1024.  Such a gradient is the one-tap GEMM dW[co][k cin_pad + ci] = G^T A3 in the bf16x3w
 * kernel (hi^T hi + hi^T lo + lo^T hi, fp32 accumulation, fixed summation order): column k cin_pad + ci of row r of A3 is row r + k - 1 of
 * channel ci where that row is a frame of row r's own sequence, and zero where it is not (the batch's ends, padded frames, gap rows, the
 * neighbouring sequence).  A3 is written in the split layout into the second of bf16x3w's two scratch buffers (3 cin_pad <= 3072): the
 * workspace is bf16x3wa's.  The bias gradient is the fp32 sum of hi + lo over the rows of G.  conv_blocks.0.conv1 at other widths,
 * residual_path and w_out stay on the exact fp32 kernels.  bf16x3w / bf16x3wa <-> bf16x3wac rebuilds no weight pack.
 * bf16x3wack: the bf16x3wac step, bit for bit in every launch but the attention's key-tiled backward: dK^T += Q^T dS (the 1 / sqrt(d) scale in the
 * epilogue), dV^T += dO^T Pd and the first stage of the position tables' gradient dE[h][r] = sum dS[., r] Q run as hi hi + hi lo + lo hi on
 * v_mfma_f32_16x16x32_bf16 with fp32 accumulation, 32 queries (rows) per MFMA.  dO and Q rows are split on their way into LDS and read as the
 * transposed operand; dS and Pd are read from the same banded fp32 buffers the query-tiled backward writes (dQ and those buffers are
 * bf16x3wac's bit for bit) and split in registers (dK, dV) or on their way into LDS (the table gradient).  The second stage of the table
 * gradient stays the ordered fp32 column sum.  Deterministic; padded keys and gap rows get the same zero dk | dv rows.  Workspace and tape are
 * bf16x3wac's: no byte more.  Switching to or from any of bf16x3w / bf16x3wa / bf16x3wac rebuilds no weight pack.
 * Legal at any time on an f32 handle, also after hificar_xfmr_finalize and between steps: once parameters have been handed over, the packs of
 * the new arithmetic are rebuilt from the handle's device copy, in stream order behind the handle's last call.  A handle whose
 * hificar_xfmr_set_precision is bf16x3 (inference only): HIFICAR_E_STATE.  An unknown value: HIFICAR_E_INVALID.
 * A tape goes back through the arithmetic that filled it: hificar_xfmr_backward / _packed on a handle whose training arithmetic is not that
 * of its last training forward return HIFICAR_E_STATE before anything is enqueued (switch back and the tape is as good as before). */
int hificar_xfmr_set_train_precision(hificar_xfmr* h, int precision);

/* Test aid: the bf16 hi | lo weight fragments ([n_block32][chunk][tap][c16][hi | lo][lane][8] and a zero tail) of a Conv1d weight w (cout,
 * cin, K odd; HOST floats; input rows cin_pad channels wide) as bf16x3 training builds them.  mode 0: the layer's own pack; 2: its data
 * gradient's (transposed, taps flipped).  how 0: the device pack's index functions run on the host (no device needed); 1: the device pack
 * kernel, over a buffer of 0xFF bytes; 2: the host pack of the inference handles, read back from the device.  out: HOST, `capacity` 16-bit
 * elements; *elems: the pack's size in elements (set even when the buffer is too small: HIFICAR_E_INVALID then). */
int hificar_debug_pack16(int cout, int cin, int cin_pad, int K, int mode, int how, const float* w, uint16_t* out, size_t capacity, size_t* elems);

/* Test aid: fp32 rows x [M][C] (HOST floats) split for the bf16x3w weight gradients: [ceil(M / 8)][C][hi 8 | lo 8] bf16, 32 bytes per (group of 8
 * rows, column); rows past M are zero bits.  lengths (M / T frame counts of sequences of T rows; NULL: dense) marks a ragged batch's padded
 * frames, pad_row (M entries, < 0: a gap row; NULL: none; not both) a packed batch's gap rows: both are written as zero bits.  how 0: the
 * device pass's index functions run on the host (no device needed); 1: the device pass, over a buffer of 0xFF bytes.  out: HOST, `capacity`
 * bytes; *bytes: the split's size (set even when the buffer is too small: HIFICAR_E_INVALID then). */
int hificar_debug_split_rows_t(int M, int C, int T, const int32_t* lengths, const int32_t* pad_row, int how, const float* x, void* out, size_t capacity,
                               size_t* bytes);

/* Test aid: fp32 rows x [M][C] (HOST floats) split for the bf16x3wac k = 3 weight gradients: [ceil(M / 8)][3 C][hi 8 | lo 8] bf16; column
 * k C + c of row r holds row r + k - 1 of channel c, and zero bits where that row is outside [0, M), a padded frame, a gap row or a row of
 * another sequence than row r (such rows are not read).  T > 0: M / T sequences of T rows, lengths their frame counts (NULL: dense); T = 0
 * (lengths NULL): one sequence of M rows.  pad_row (M entries, < 0: a gap row; not with lengths): a packed batch, T is not used.  how, out,
 * capacity, *bytes: as hificar_debug_split_rows_t. */
int hificar_debug_split_taps_t(int M, int C, int T, const int32_t* lengths, const int32_t* pad_row, int how, const float* x, void* out, size_t capacity,
                               size_t* bytes);

/* Every float tensor of the state_dict (reference names and layouts, the batch norms' running_mean / running_var included; n = all of them,
 * each once) from DEVICE memory.  The handle copies them and rebuilds every derived form on the device, on `stream`: the GEMM packs (the
 * q | k | v weight of 3 hidden_dim rows and w_o's transpose among them), their data-gradient packs, and the eval-mode fold of every batch norm
 * into its conv — hificar_xfmr_forward sees the new weights too.  Call it after every optimizer step (and before the first
 * hificar_xfmr_forward_train).  A list that is refused leaves the handle exactly as it was, as hificar_bigru_set_parameters_device. */
int hificar_xfmr_set_parameters_device(hificar_xfmr* h, const char* const* names, const float* const* data, int n, void* stream);

/* The gradient buffer: hificar_xfmr_grad_floats(h) floats; tensor i of hificar_xfmr_grad_count(h) has the reference's state_dict name
 * (name96: at least 96 bytes) and layout — w_q / w_k / w_v (8, F, d), w_o (8, d, F), relative_positional.embeddings (8, 199, d, 1), conv
 * weights (F, C, 3) — at `offset` floats, `numel` long.  Same contract as hificar_grad_info. */
int hificar_xfmr_grad_count(hificar_xfmr* h);
int hificar_xfmr_grad_info(hificar_xfmr* h, int i, char* name96, int64_t* offset, int64_t* numel);
int64_t hificar_xfmr_grad_floats(hificar_xfmr* h);

/* Bytes of the tape (what a training forward keeps for its backward pass: the input rows; per batch norm its conv's raw output rows and the
 * statistics; per ResBlock its two ReLU outputs; per encoder layer its input rows, q | k | v, the attention's output rows and L = m + log l
 * per (head, query), both pre-LayerNorm rows, norm1's output and the feed-forward's hidden rows; dropout masks are regenerated, not stored)
 * and of the scratch shared by hificar_xfmr_forward_train and hificar_xfmr_backward; the B frame counts of a ragged forward). */
size_t hificar_xfmr_tape_bytes(const hificar_xfmr* h, int B, int T);
size_t hificar_xfmr_train_workspace_bytes(hificar_xfmr* h, int B, int T);

/* Transformer.forward in train() mode: x (B, in_channels, T) -> out (B, out_channels, T), device fp32.
 * Batch norms: per-channel mean and BIASED variance over the B T frames (two-pass variance); bn_batch_stats receives 2 hidden_dim device
 * floats (mean | variance) per BatchNorm1d in registration order — conv_blocks.0.bn1, .bn2, (.res_norm when in_channels != hidden_dim),
 * conv_blocks.1.bn1, ... : 7 of them, or 6 — and the caller updates the running statistics as torch.nn.BatchNorm1d does.
 * Dropout: element e of site s is kept when u(seed, offset, s, e) >= dropout_p and scaled by 1 / (1 - dropout_p); u is the counter-based
 * generator of hificar_bigru_forward_train with the key mix(seed ^ mix(128 offset + s)) (numpy restatement:
 * articulatory_amd.utils.synth.xfmr_dropout_mask), `offset` the caller's count of training forwards.  Sites of encoder layer l: 4 l + 0 the
 * attention probabilities, e = ((b 8 + h) T + q) 199 + (k - q + 99) (only in-band probabilities exist); 4 l + 1 dropout1, 4 l + 2 the
 * feed-forward's hidden rows, 4 l + 3 dropout2, e = the element's index in the (B, T, C) tensor.  dropout_p = 0 is the identity.
 * B * T >= 2.  tape / workspace: 256-byte aligned device memory of at least the sizes above; what they hold on entry does not matter; the
 * tape is the caller's until hificar_xfmr_backward ran.  tape = NULL (tape_bytes ignored): the same arithmetic and outputs without a tape. */
int hificar_xfmr_forward_train(hificar_xfmr* h, const float* x, float* out, float* bn_batch_stats, int B, int T, float dropout_p, uint64_t seed,
                               uint64_t offset, void* tape, size_t tape_bytes, void* workspace, size_t workspace_bytes, void* stream);

/* The same step on a ragged batch of whole utterances: sequence b has lengths[b] frames (0 .. T; M = their sum >= 2) of x (B, in_channels, T);
 * what x holds past them is never used (NaN included), and neither is what the tape and the workspace hold on entry.
 *   convs (k = 3)  a sequence sees zero padding at its own end (as hificar_xfmr_forward does with lengths)
 *   batch norms    mean and biased variance over the M valid rows (two-pass); bn_batch_stats as above (the caller's running variance takes
 *                  M / (M - 1))
 *   attention      a query's keys lie within +-99 and below its sequence's own length; queries at or past the length do not exist
 *   LayerNorm, Linear, feed-forward   per row: valid rows exactly as above
 *   dropout        element e is the index in the PADDED (B, T, C) tensor, and ((b 8 + h) T + q) 199 + (k - q + 99) for the probabilities,
 *                  as above: the masks depend on T, not only on the lengths
 *   out            out[b, :, lengths[b]:] is exactly zero
 * lengths: device int32[B].  lengths_host: the same values on the host, required: each is checked against 0 .. T and their sum against >= 2
 * before anything is enqueued (HIFICAR_E_INVALID otherwise).  The tape records the lengths and M, so hificar_xfmr_backward takes no new
 * argument and cannot be run with other lengths than its forward: on such a tape it ignores dout on padded frames, whatever it holds, writes
 * dx = 0 there, and every weight, bias, d gamma / d beta and relative-position table gradient sums valid frames only (the batch norms'
 * backward divides by the same M).  With all lengths = T every result is bitwise that of hificar_xfmr_forward_train.  Deterministic (no
 * atomics).  tape = NULL: the forward-only form, as above.
 * The GEMMs still run over all B T rows (zeros in the padded rows mask them); the attention kernels skip the 64-frame tiles that hold
 * padding only.  Padding costs GEMM time, not correctness. */
int hificar_xfmr_forward_train_ragged(hificar_xfmr* h, const float* x, const int32_t* lengths, const int32_t* lengths_host, float* out,
                                      float* bn_batch_stats, int B, int T, float dropout_p, uint64_t seed, uint64_t offset, void* tape,
                                      size_t tape_bytes, void* workspace, size_t workspace_bytes, void* stream);

/* dout (B, out_channels, T) -> grads (hificar_xfmr_grad_floats floats: written, not accumulated) and, with dx non-NULL, the input's
 * gradient (B, in_channels, T).  The weights must be those of the forward that filled the tape.  Deterministic, as above.  A tape of
 * hificar_xfmr_forward_train_ragged: see there. */
int hificar_xfmr_backward(hificar_xfmr* h, const float* dout, int B, int T, const void* tape, size_t tape_bytes, float* grads, float* dx,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- The ragged step, packed: the same function as hificar_xfmr_forward_train_ragged + hificar_xfmr_backward — the same masks (dropout
 * elements are those of the PADDED tensors, so they depend on T), the same batch statistics over the M valid rows, the same attention — with
 * every GEMM, data gradient and weight gradient over Mp rows instead of B T; only the order of the sums over rows differs (results agree
 * to rounding, not bitwise).  Inside, sequence b's frames are rows row0[b] .. row0[b] + lengths[b] - 1, one zero gap row follows every
 * sequence (what a k = 3 conv over one run of rows needs to see each sequence's own end), and
 *     Mp = sum over b of (lengths[b] + 1), rounded up to a multiple of 256        (hificar_xfmr_packed_rows; the tail rows are gap rows)
 * x, out, dout and dx keep the padded (B, C, T) layout: out and dx are exactly zero on padded frames, x and dout are never read there (NaN
 * included).  The tape and the workspace are sized by Mp (below), not by B T.  Deterministic, no atomics; what tape, workspace and outputs
 * hold on entry does not matter.  Debug taps are delivered in the padded (B, T, width) layout, zeros on padded frames. ---- */

/* Mp of a batch, on the host; 0 for invalid input: a null pointer, B or T < 1, a length outside 0 .. T, fewer than two frames in all, or
 * Mp * 3072 >= 2^31. */
int hificar_xfmr_packed_rows(int B, int T, const int32_t* lengths_host);

/* Bytes of a packed tape and of the scratch shared by the packed forward and backward, for B sequences in Mp rows (T plays no part; 0 for
 * an Mp that hificar_xfmr_packed_rows cannot return). */
size_t hificar_xfmr_tape_bytes_packed(const hificar_xfmr* h, int B, int Mp);
size_t hificar_xfmr_train_workspace_bytes_packed(hificar_xfmr* h, int B, int Mp);

/* hificar_xfmr_forward_train_ragged's arguments and checks (lengths_host required: each length in 0 .. T, their sum >= 2, and
 * Mp * 3072 < 2^31, all before anything is enqueued).  tape = NULL: the forward-only form. */
int hificar_xfmr_forward_train_packed(hificar_xfmr* h, const float* x, const int32_t* lengths, const int32_t* lengths_host, float* out,
                                      float* bn_batch_stats, int B, int T, float dropout_p, uint64_t seed, uint64_t offset, void* tape,
                                      size_t tape_bytes, void* workspace, size_t workspace_bytes, void* stream);

/* The backward of a packed tape: hificar_xfmr_backward's arguments plus the forward's lengths on the host, which give Mp.  A separate entry
 * point rather than a tape that hificar_xfmr_backward recognises: the tape's header lives on the device, and reading it back would cost
 * every backward a synchronisation.  Instead the handle remembers, by address, the packed tapes it filled and their lengths (a dense or
 * ragged forward into the same memory forgets the entry), so before anything is enqueued
 *   hificar_xfmr_backward_packed on a tape that is not a packed tape of this handle      HIFICAR_E_STATE
 *   hificar_xfmr_backward on a packed tape                                               HIFICAR_E_STATE
 *   hificar_xfmr_backward_packed with another B, T or other lengths than the forward's   HIFICAR_E_INVALID
 * and the tape stays usable for the right call.  A tape is known by its address: one copied elsewhere is not recognised. */
int hificar_xfmr_backward_packed(hificar_xfmr* h, const float* dout, const int32_t* lengths_host, int B, int T, const void* tape, size_t tape_bytes,
                                 float* grads, float* dx, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Speech representation: the HuBERT encoder of the "large" family (the published architecture as the `transformers` library's
 * HubertModel states it with feat_extract_norm = "layer", do_stable_layer_norm = True, feat_proj_layer_norm = True), waveforms at 16 kHz ->
 * hidden states at 50 Hz, the front end of the reference's SSL inversion models (egs/ema/voc1/local/predict_ema.py puts hubert_large_ll60k's
 * last hidden state, stretched by 4, in front of the BiGRU).  Inference only; exact fp32 unless hificar_hubert_set_precision says otherwise.
 *   normalisation  per utterance (x - mean) / sqrt(var + norm_eps) over its own samples, population variance, applied as layer 0 reads
 *   extractor      seven Conv1d (kernels 10, 3, 3, 3, 3, 2, 2; strides 5, 2, 2, 2, 2, 2, 2; conv_dim channels), each + LayerNorm over channels
 *                  (eps 1e-5) + GELU (erf): layer 0 in a kernel of its own, layers 1 - 6 on the conv engine as stride-1 convs over rows of two
 *                  positions, in sub-batches of utterances (the workspace holds a sub-batch's layer-0 rows, never the batch's)
 *   projection     LayerNorm(conv_dim) + Linear(conv_dim, hidden_size)
 *   positional     Conv1d(hidden, hidden, 128, padding 64, groups 16) without its last frame, + bias, GELU, added to the stream
 *   layers         x += W_o attn(LN(x)); x += W_2 GELU(W_1 LN(x)); heads of 64 channels, full softmax attention over the utterance's own frames
 *   output         layer = -1: LayerNorm of the last layer's stream (last_hidden_state); layer = k in 0 .. N - 1: the stream in front of
 *                  layer k (hidden_states[k] of output_hidden_states = True); layers k and above are then not run
 * Limits: conv_dim a multiple of 32 in 32 .. HIFICAR_HUBERT_MAX_CONV; hidden_size one of 128, 256, 512, 768, 1024 (16 positional groups of 8 ..
 * 64 channels, LayerNorm rows of at most 1024); num_attention_heads = hidden_size / 64; intermediate_size a multiple of 32 in 32 ..
 * HIFICAR_HUBERT_MAX_FFN; 1 .. HIFICAR_HUBERT_MAX_LAYERS layers.  Not built (the binding refuses them): group-norm extractors, post-LN encoders
 * (HuBERT-base, WavLM-base), the gated relative position bias under bf16x3a, training, dropout, spec-augment.
 * Every utterance of a batch is computed as if alone, bit for bit: the conv engine runs with split-K off, every other sum has one order.
 *
 * Opt-in bf16x3 (HIFICAR_PREC_BF16X3): every GEMM on the conv engine — extractor layers 1 - 6, the projection, q | k | v, out_proj,
 * intermediate_dense, output_dense — as x w ~ hi hi + hi lo + lo hi on bf16 MFMAs with fp32 accumulation, hi = bf16(x), lo = bf16(x - hi).
 * The producers of those GEMMs' inputs (layer 0, the LayerNorms, the attention, the GELU pass) write split rows directly; the waveform
 * statistics, layer 0, every LayerNorm and GELU, the positional conv, the attention, biases, residual adds and the residual stream stay fp32.
 * Opt-in bf16x3a (HIFICAR_PREC_BF16X3A): bf16x3, and the attention's two products (Q K^T, P V) in the same three-term form on
 * v_mfma_f32_16x16x32_bf16; the softmax statistics stay fp32.  Both keep "every utterance as if alone, bit for bit" and the workspace's size.
 *
 * WavLM (hificar_hubert_set_rel_bias): the same encoder with the gated relative position bias of the library's WavLMAttention,
 *     S[q, k] = Q[q] . K[k] / sqrt(d) + gate[b, h, q] bias[h][bucket(k - q)],
 * gate = a (b const[h] - 1) + 2 with a, b the sigmoids of the two four-sums of gru_rel_pos_linear over the head's 64 channels of the layer's
 * attention input (the LayerNorm's fp32 output, taken from the LayerNorm kernel's registers in either arithmetic: an f32 and a bf16x3 handle
 * form the same gates, bit for bit).  The (heads, T, T) bias is never formed: the attention reads one table per head.
 * --------------------------------------------------------------------------------------------------------------------------- */
#define HIFICAR_HUBERT_MAX_CONV 1024
#define HIFICAR_HUBERT_MAX_BUCKETS 4096
#define HIFICAR_HUBERT_MAX_DISTANCE 65536
#define HIFICAR_HUBERT_MAX_HIDDEN 1024
#define HIFICAR_HUBERT_MAX_FFN 8192
#define HIFICAR_HUBERT_MAX_LAYERS 48
#define HIFICAR_HUBERT_HEAD_DIM 64
#define HIFICAR_HUBERT_MIN_SAMPLES 400

typedef struct hificar_hubert_config {
    int32_t conv_dim;            /* every extractor layer's channels */
    int32_t hidden_size;
    int32_t num_hidden_layers;
    int32_t num_attention_heads; /* hidden_size / 64 */
    int32_t intermediate_size;
    int32_t conv_bias;           /* the extractor convs have biases */
    int32_t normalize;           /* per-utterance waveform normalisation in front of layer 0 */
    float layer_norm_eps;        /* every LayerNorm but the extractor's (1e-5 there, torch.nn.LayerNorm's default) */
    float norm_eps;              /* the waveform normalisation's eps */
} hificar_hubert_config;

typedef struct hificar_hubert hificar_hubert;

/* An empty model for this configuration.  Touches no device. */
int hificar_hubert_create(const hificar_hubert_config* cfg, hificar_hubert** out);

/* One tensor by its HubertModel state_dict name: "feature_extractor.conv_layers.<i>.conv.weight" (C, 1 | C, k), ".conv.bias" (conv_bias),
 * ".layer_norm.weight" / ".bias"; "feature_projection.layer_norm.*" (C), "feature_projection.projection.weight" (H, C), ".bias";
 * "encoder.pos_conv_embed.conv.weight_g" (1, 1, 128), ".weight_v" (H, H / 16, 128) — the weight norm over dim 2, folded in double by
 * hificar_hubert_finalize — and ".bias"; "encoder.layer_norm.*"; per layer "encoder.layers.<l>.attention.{q,k,v,out}_proj.weight" (H, H) / ".bias",
 * ".layer_norm.*", ".feed_forward.intermediate_dense.weight" (I, H) / ".bias", ".feed_forward.output_dense.weight" (H, I) / ".bias",
 * ".final_layer_norm.*".  data: HOST pointer to contiguous fp32; the caller keeps ownership. */
int hificar_hubert_set_weight(hificar_hubert* h, const char* name, const float* data, const int64_t* shape, int ndim);

/* The arithmetic of the handle's GEMMs: HIFICAR_PREC_F32 (the default), HIFICAR_PREC_BF16X3 or HIFICAR_PREC_BF16X3A (above).  Between
 * hificar_hubert_create and hificar_hubert_finalize only (finalize packs the weights for one arithmetic): HIFICAR_E_STATE afterwards; any
 * other value, the training-only ones included, HIFICAR_E_INVALID.  Touches no device.  hificar_hubert_workspace_bytes answers for the
 * arithmetic set when it is called.  A handle that is not f32 refuses the debug tap "extractor.0" with HIFICAR_E_STATE (those rows exist as
 * split bf16 rows only). */
int hificar_hubert_set_precision(hificar_hubert* h, int precision);

/* Switches the gated relative position bias on (WavLM), between hificar_hubert_create and hificar_hubert_finalize (HIFICAR_E_STATE
 * afterwards).  bucket_of_distance: HOST, 2 max_distance + 1 entries, bucket_of_distance[d + max_distance] = bucket(d) in 0 .. num_buckets - 1
 * for d in -max_distance .. max_distance; distances beyond are clamped, which is exact for the library's bucket function (its last bucket
 * starts at max_distance).  The caller computes the map — the library takes a float32 logarithm there, and this side never evaluates one.
 * HIFICAR_E_INVALID: num_buckets odd, under 2 or over HIFICAR_HUBERT_MAX_BUCKETS; max_distance outside 1 .. HIFICAR_HUBERT_MAX_DISTANCE; an
 * entry out of range; a handle set to HIFICAR_PREC_BF16X3A (and hificar_hubert_set_precision(BF16X3A) after this call: the bf16 attention
 * kernel has no bias term).  Afterwards hificar_hubert_set_weight also takes — and hificar_hubert_finalize asks for —
 * "encoder.layers.0.attention.rel_attn_embed.weight" (num_buckets, heads) and, per layer, "encoder.layers.<l>.attention.gru_rel_pos_linear.weight"
 * (8, 64), ".bias" (8) and "encoder.layers.<l>.attention.gru_rel_pos_const" (1, heads, 1, 1); finalize folds embedding and map into one fp32
 * table per head, [heads][2 max_distance + 1].  hificar_hubert_workspace_bytes grows by one layer's gates, B heads Tmax floats; the debug tap
 * "gate.<l>" (B, heads, Tmax) holds the gates layer l used.  Touches no device.  Without this call a handle computes, launches and
 * reports exactly what it did before the call existed. */
int hificar_hubert_set_rel_bias(hificar_hubert* h, int num_buckets, int max_distance, const int32_t* bucket_of_distance);

/* Checks that every tensor arrived, folds the weight norm, re-lays the strided convs' weights as windows of two positions, packs q | k | v
 * as one GEMM, uploads.  Synchronises the device once. */
int hificar_hubert_finalize(hificar_hubert* h);

/* Frames of an utterance of L samples: (L - 400) / 320 + 1 (integer division); 0 for L < 400. */
int hificar_hubert_frames(const hificar_hubert* h, int L);

/* Bytes of device scratch hificar_hubert_forward needs for B utterances of at most L samples; 0: the shape is refused.  The extractor runs
 * over sub-batches of utterances whose layer-0 rows take at most 512 MiB (one utterance's, if those are more), so the figure grows with B
 * by the 50-Hz rows only: conv_dim + 4 hidden_size + max(3 hidden_size, intermediate_size) floats per frame. */
size_t hificar_hubert_workspace_bytes(const hificar_hubert* h, int B, int L);

/* wav (B, L) device fp32, zero-padded; lengths: DEVICE int32[B] sample counts or NULL (every utterance has L); lengths_host: the same on the
 * host or NULL — given, every entry is checked (400 <= l <= L) before anything is enqueued; not given, a length is clamped into 0 .. L and an
 * utterance under 400 samples has no frames.  out: (B, hidden_size, Tmax), Tmax = hificar_hubert_frames(h, L), exactly zero from an
 * utterance's own frame count on.  layer: -1 or 0 .. num_hidden_layers - 1 (above).  workspace: 256-byte aligned,
 * hificar_hubert_workspace_bytes(h, B, L) bytes; what it holds on entry does not matter.  L < 400: HIFICAR_E_INVALID. */
int hificar_hubert_forward(hificar_hubert* h, const float* wav, const int32_t* lengths, const int32_t* lengths_host, float* out, int B, int L,
                           int layer, void* workspace, size_t workspace_bytes, void* stream);

/* Test aid: the following forwards also copy the named intermediate into dst (device, `capacity` floats).  Names: "extractor.0" (B, T0,
 * conv_dim) with T0 = (L - 10) / 5 + 1, "extract_features" (B, Tmax, conv_dim: extractor layer 6's output), "feature_projection", "pos_conv"
 * (GELU(conv + bias) alone) and "layers.<l>" (the stream behind layer l), each (B, Tmax, hidden_size).  Rows past an utterance's frames hold
 * whatever the workspace held.  name = NULL forgets every tap, dst = NULL that one. */
int hificar_hubert_debug_tap(hificar_hubert* h, const char* name, float* dst, size_t capacity);

/* Test aid: the extractor's sub-batches hold `utterances` utterances (0: as many as the 512-MiB budget allows, the default) from the next
 * hificar_hubert_workspace_bytes / hificar_hubert_forward on.  Results do not depend on it. */
int hificar_hubert_debug_sub_batch(hificar_hubert* h, int utterances);

/* The model's engine, for hificar_profile_begin / hificar_profile_end. */
hificar_engine* hificar_hubert_engine(hificar_hubert* h);

void hificar_hubert_destroy(hificar_hubert* h);

/* ---------------------------------------------------------------------------------------------------------------------------
 * A linear head on device features: y[b, :, t] = coef x[b, :, t] + intercept over (B, in, T) -> (B, out, T) — the fitted linear regression
 * the reference's egs/ema/voc1/local/linear_inference.py applies to hidden_states[9] of wavlm_large.  The one-tap GEMM every Linear of this
 * library is, on the conv engine, exact fp32, split-K off: every utterance is computed as if alone, bit for bit.
 * --------------------------------------------------------------------------------------------------------------------------- */
#define HIFICAR_LINEAR_MAX_IN 8192
#define HIFICAR_LINEAR_MAX_OUT 1024

typedef struct hificar_linear hificar_linear;

/* coef: HOST (out_features, in_features) fp32, row-major (sklearn's coef_); intercept: HOST (out_features).  Packs and uploads the weights:
 * runs on the current device and synchronises it once. */
int hificar_linear_create(int in_features, int out_features, const float* coef, const float* intercept, hificar_linear** out);

/* Bytes of device scratch hificar_linear_forward needs for B sequences of at most T frames; 0: the shape is refused. */
size_t hificar_linear_workspace_bytes(const hificar_linear* h, int B, int T);

/* x (B, in_features, T) device fp32; lengths: DEVICE int32[B] frame counts (clamped into 0 .. T) or NULL (every sequence has T);
 * out (B, out_features, T), exactly zero from a sequence's own length on.  workspace: 256-byte aligned. */
int hificar_linear_forward(hificar_linear* h, const float* x, const int32_t* lengths, float* out, int B, int T, void* workspace, size_t workspace_bytes,
                           void* stream);

/* The head's engine, for hificar_profile_begin / hificar_profile_end. */
hificar_engine* hificar_linear_engine(hificar_linear* h);

void hificar_linear_destroy(hificar_linear* h);

#ifdef __cplusplus
}
#endif
#endif /* HIFICAR_H */
