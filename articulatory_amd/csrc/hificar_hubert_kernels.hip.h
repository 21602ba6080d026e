// Kernels of the HuBERT encoder ("large" family: layer-norm extractor, stable layer norm) that are not GEMMs on the conv engine.
//   hubert_stats_kernel    per utterance, mean and 1 / sqrt(var + eps) of its own samples (population variance), two passes in double
//   hubert_frames_kernel   the 50-Hz frame count of every utterance, (l - 400) / 320 + 1, for every kernel behind the extractor
//   hubert_conv0_kernel    extractor layer 0: normalised samples -> Conv1d(1 -> C, k 10, s 5) + LayerNorm(C) + GELU, one wave per output row
//   hubert_ln_kernel       LayerNorm(F) with the config's eps, optionally followed by GELU (extractor layers 1 - 6); source and destination
//                          may have different rows per sequence
//   hubert_gelu_kernel     GELU in place on the feed-forward's hidden rows
//   hubert_posconv_kernel  the grouped 128-tap positional conv on v_mfma_f32_16x16x4_f32: x + GELU(conv(x) + b)
//   hubert_attn_kernel     full softmax attention over the utterance's own keys: xfmr_attn_kernel's transposed-MFMA plan without band,
//                          table or positional LDS region
// Exact fp32 arithmetic throughout (GELU in its erf form).  Every sum's order depends on the utterance alone: no atomics, no split reductions
// whose shape depends on the batch.  The bf16x3 forward's instantiations (hubert_conv0_kernel<true>, hubert_ln_kernel<GELU, true>,
// hubert_gelu_split_kernel, hubert_attn_kernel<D, true>) differ in the FORMAT they store — split rows for the bf16x3 GEMM that reads them
// (xfmr_store_split) — not in how they compute.
// WavLM's gated relative position bias (hificar_hubert_set_rel_bias): hubert_ln_kernel<false, SPLIT, true> also forms the attention's gates
// from the normalised row it holds in registers, and hubert_attn_kernel<D, SPLIT, true> adds gate[q] bias_d[h][k - q] to every score.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hificar_xfmr_kernels.hip.h"

namespace hificar {

constexpr int kHubK0 = 10, kHubS0 = 5;      // extractor layer 0: kernel and stride
constexpr int kHubPosTaps = 128;            // num_conv_pos_embeddings
constexpr int kHubPosGroups = 16;           // num_conv_pos_embedding_groups
constexpr int kHubPosTR = 128;              // output rows per workgroup of the positional conv: four waves of 32
constexpr int kHubHeadDim = 64;

__device__ __forceinline__ float hubert_gelu(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }

// One workgroup per utterance: stats[b] = (mean, 1 / sqrt(var + eps)) as doubles over wav[b, :l].  The summation plan of frontend_stats_kernel:
// a thread sums its samples in index order, a wave's lanes by a butterfly, the four waves in wave order.
__global__ __launch_bounds__(256) void hubert_stats_kernel(const float* __restrict__ wav, const int* __restrict__ lengths, double* __restrict__ stats, int L,
                                                           double eps) {
    __shared__ double part[4];
    __shared__ double total;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int l = lengths ? min(max(lengths[b], 0), L) : L;
    const float* const xb = wav + (size_t)b * L;
    double mean = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
        double acc = 0.0;
        for (int e = tid; e < l; e += 256) {
            const double v = (double)xb[e];
            acc += pass == 0 ? v : (v - mean) * (v - mean);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
        if ((tid & 63) == 0) part[tid >> 6] = acc;
        __syncthreads();
        if (tid == 0) total = ((part[0] + part[1]) + part[2]) + part[3];
        __syncthreads();
        const double s = total;
        __syncthreads();
        if (pass == 0) mean = l > 0 ? s / (double)l : 0.0;
        else if (tid == 0) {
            stats[2 * b] = mean;
            stats[2 * b + 1] = l > 0 ? 1.0 / sqrt(s / (double)l + eps) : 0.0;
        }
    }
}

// frames[b] = (l - 400) / 320 + 1 for l >= 400 samples (the seven convs' lengths composed), 0 below; l clamped into 0 .. L
__global__ __launch_bounds__(256) void hubert_frames_kernel(const int* __restrict__ lengths, int* __restrict__ frames, int B, int L) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const int l = lengths ? min(max(lengths[b], 0), L) : L;
    frames[b] = l >= 400 ? (l - 400) / 320 + 1 : 0;
}

// SPLIT: the row goes out as split rows instead of fp32: hi at ys, lo 2 FS bytes behind it (FS = F: a row of its own [hi: F | lo: F];
// FS = 2 F: one position's half of a window row [hi: 2 F | lo: 2 F], hificar_hubert.hip.inc).  F % 8 == 0 there: lanes i and i ^ 1 hold
// eight adjacent channels and are active together.
// What the gate of WavLM's relative position bias reads (hubert_ln_row<SPLIT, true>): gru_rel_pos_linear (8, 64) and its bias (8),
// gru_rel_pos_const (heads), and where the row's gates go: out[head * stride], one float per head.
struct HubertGateArgs {
    const float* w;
    const float* b;
    const float* c;
    float* out;
    size_t stride;
};

// GATE: the gates of the row, from the normalised values before they are stored — the same registers in either format, so an f32 and a bf16x3
// model form the same bits.  F is a multiple of 64 there (heads of 64 channels): the float4 of index i = lane + 64 j belongs to head i / 16 =
// lane / 16 + 4 j, so a head's 64 channels lie in one 16-lane group of one j.  A lane forms its four channels' part of the eight projections
// (channels in order), sums them as (p0 + p1) + (p2 + p3) and (p4 + p5) + (p6 + p7), and the group adds its 16 lanes by a butterfly (xor 1,
// 2, 4, 8); the biases go on last.  gate = a (b const - 1) + 2 with a, b the sigmoids of the two sums.
template <bool SPLIT = false, bool GATE = false>
__device__ __forceinline__ void hubert_ln_row(float4 (&v)[4], int lane, int nv, int F, float eps, const float* gamma, const float* beta, bool gelu,
                                              float* yrow, char* ys = nullptr, int FS = 0, const HubertGateArgs* gate = nullptr) {
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (lane + 64 * j < nv) sum += (v[j].x + v[j].y) + (v[j].z + v[j].w);
    const float mean = xfmr_wave_sum(sum) / (float)F;
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (lane + 64 * j >= nv) continue;
        const float a = v[j].x - mean, bb = v[j].y - mean, cc = v[j].z - mean, d = v[j].w - mean;
        sq += (a * a + bb * bb) + (cc * cc + d * d);
    }
    const float rstd = 1.f / sqrtf(xfmr_wave_sum(sq) / (float)F + eps);
    const float4* gm = reinterpret_cast<const float4*>(gamma);
    const float4* bt = reinterpret_cast<const float4*>(beta);
    float4* y = reinterpret_cast<float4*>(yrow);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = lane + 64 * j;
        if (i >= nv) continue;
        const float4 gv = gm[i], bv = bt[i];
        float4 r = make_float4((v[j].x - mean) * rstd * gv.x + bv.x, (v[j].y - mean) * rstd * gv.y + bv.y, (v[j].z - mean) * rstd * gv.z + bv.z,
                               (v[j].w - mean) * rstd * gv.w + bv.w);
        if (gelu) r = make_float4(hubert_gelu(r.x), hubert_gelu(r.y), hubert_gelu(r.z), hubert_gelu(r.w));
        if constexpr (SPLIT) xfmr_store_split(ys, FS, 4 * i, i & 1, 1, r.x, r.y, r.z, r.w, true);
        else y[i] = r;
        if constexpr (GATE) v[j] = r;  // (kept for the gates below: the wave leaves the loop before it shuffles)
    }
    if constexpr (GATE) {
        const int c = lane & 15;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (64 * j >= nv) break;  // (wave-uniform)
            const bool in = lane + 64 * j < nv;  // (nv is a multiple of 16: a 16-lane group is in or out together)
            float pk[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float4 w = reinterpret_cast<const float4*>(gate->w + k * kHubHeadDim)[c];
                pk[k] = in ? fmaf(w.w, v[j].w, fmaf(w.z, v[j].z, fmaf(w.y, v[j].y, w.x * v[j].x))) : 0.f;
            }
            float sa = (pk[0] + pk[1]) + (pk[2] + pk[3]), sb = (pk[4] + pk[5]) + (pk[6] + pk[7]);
#pragma unroll
            for (int m = 1; m <= 8; m <<= 1) {
                sa += __shfl_xor(sa, m);
                sb += __shfl_xor(sb, m);
            }
            if (in && c == 0) {
                const int head = (lane >> 4) + 4 * j;
                sa += (gate->b[0] + gate->b[1]) + (gate->b[2] + gate->b[3]);
                sb += (gate->b[4] + gate->b[5]) + (gate->b[6] + gate->b[7]);
                const float ga = 1.f / (1.f + expf(-sa)), gb = 1.f / (1.f + expf(-sb));
                gate->out[(size_t)head * gate->stride] = ga * (gb * gate->c[head] - 1.f) + 2.f;
            }
        }
    }
}

// where position t of a sequence whose rows start at `base` (pitch: P positions of C channels, 4 C bytes each in either format) keeps its hi
// half in the window layout: window t / 2 is [hi: 2 C bf16 | lo: 2 C bf16], position t's C channels at (t & 1) C of each half
__device__ __forceinline__ char* hubert_window_ptr(char* base, int t, int C) { return base + (size_t)(t >> 1) * 8 * C + (t & 1) * 2 * C; }

// Extractor layer 0.  One wave per output row (position t of sequence b of this sub-batch): the row's ten samples are normalised in double
// with the utterance's statistics (stats null: taken as they are) and rounded once; samples at or past the utterance's length are zeros, as
// the library's padding after normalisation.  The C outputs are formed (taps in order), normalised over C (eps 1e-5, torch.nn.LayerNorm's
// default), activated and stored once.  Rows T0 .. P - 1 of a sequence (the slack that makes its rows a whole number of stride-2 windows)
// are zeros.  w: [10][C]; C a multiple of 4, at most 1024.  SPLIT (the bf16x3 forward): y holds the same rows as split window rows, layer
// 1's operand (hubert_window_ptr; C a multiple of 8; zero rows are zero bits in either format).
struct HubertConv0Params {
    const float* wav;      // [B][L], this sub-batch's first utterance
    const int* lengths;    // this sub-batch's, or null
    const double* stats;   // this sub-batch's [mean, rstd], or null
    const float* w;        // [10][C]
    const float* bias;     // [C] (zeros without conv_bias)
    const float* gamma;
    const float* beta;
    float* y;              // [nseq][P][C]
    int nseq, L, T0, P, C;
};

template <bool SPLIT = false>
__global__ __launch_bounds__(256) void hubert_conv0_kernel(const HubertConv0Params p) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long long)p.nseq * p.P) return;
    const int b = (int)(row / p.P), t = (int)(row - (long long)b * p.P);
    const int nv = p.C >> 2;
    float* const yrow = p.y + (size_t)row * p.C;
    char* const ys = SPLIT ? hubert_window_ptr(reinterpret_cast<char*>(p.y + (size_t)b * p.P * p.C), t, p.C) : nullptr;
    if (t >= p.T0) {
        if constexpr (SPLIT) {  // nv / 2 pieces of 16 bytes in each half (2 C bytes), the lo half 4 C bytes behind the hi half
            for (int i = lane; i < nv; i += 64)
                *reinterpret_cast<uint4*>(ys + (i < nv / 2 ? 16 * i : 4 * p.C + 16 * (i - nv / 2))) = make_uint4(0u, 0u, 0u, 0u);
        } else {
            for (int i = lane; i < nv; i += 64) reinterpret_cast<float4*>(yrow)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return;
    }
    const int l = p.lengths ? min(max(p.lengths[b], 0), p.L) : p.L;
    const double mean = p.stats ? p.stats[2 * b] : 0.0, rstd = p.stats ? p.stats[2 * b + 1] : 1.0;
    float xs[kHubK0];
#pragma unroll
    for (int k = 0; k < kHubK0; ++k) {
        const int s = kHubS0 * t + k;  // (< L: t < T0)
        xs[k] = s < l ? (float)(((double)p.wav[(size_t)b * p.L + s] - mean) * rstd) : 0.f;
    }
    float4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = lane + 64 * j;
        v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i >= nv) continue;
        float4 a = reinterpret_cast<const float4*>(p.bias)[i];
#pragma unroll
        for (int k = 0; k < kHubK0; ++k) {
            const float4 w = reinterpret_cast<const float4*>(p.w + (size_t)k * p.C)[i];
            a.x = fmaf(w.x, xs[k], a.x);
            a.y = fmaf(w.y, xs[k], a.y);
            a.z = fmaf(w.z, xs[k], a.z);
            a.w = fmaf(w.w, xs[k], a.w);
        }
        v[j] = a;
    }
    hubert_ln_row<SPLIT>(v, lane, nv, p.C, 1e-5f, p.gamma, p.beta, true, yrow, ys, 2 * p.C);
}

// LayerNorm(F) + optional GELU, one wave per row: row t of sequence b is read at x[(b Tin + t) F] and written at y[(b Tout + t) F], t < T.
// Rows at or past a sequence's length (lengths non-null) are left alone.  x and y may be the same buffer when Tin == Tout.  F <= 1024, F % 4 == 0.
// SPLIT (the bf16x3 forward; F % 8 == 0): y takes the rows as split rows only, 4 F bytes each like the fp32 row, so x and y may still be the
// same buffer when Tin == Tout (a wave holds its whole row before it stores).  window: as split window rows of two positions
// (hubert_window_ptr, Tout positions per sequence), the next extractor layer's operand — a position's bytes interleave with its
// neighbour's there, so y must NOT be x.
struct HubertLnParams {
    const float* x;
    const float* gamma;
    const float* beta;
    const int* lengths;
    float* y;
    int B, T, Tin, Tout, F;
    float eps;
    int window = 0;
    // GATE: gru_rel_pos_linear's weight (8, 64) and bias (8), gru_rel_pos_const (heads), and gates (B, heads, T): row t of sequence b writes
    // gates[(b heads + head) T + t]
    const float* gate_w = nullptr;
    const float* gate_b = nullptr;
    const float* gate_c = nullptr;
    float* gates = nullptr;
};

template <bool GELU, bool SPLIT = false, bool GATE = false>
__global__ __launch_bounds__(256) void hubert_ln_kernel(const HubertLnParams p) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long long)p.B * p.T) return;
    const int b = (int)(row / p.T), t = (int)(row - (long long)b * p.T);
    const int len = p.lengths ? min(max(p.lengths[b], 0), p.T) : p.T;
    if (t >= len) return;
    const int nv = p.F >> 2;
    const float4* x = reinterpret_cast<const float4*>(p.x + ((size_t)b * p.Tin + t) * p.F);
    float4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = lane + 64 * j;
        v[j] = i < nv ? x[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    HubertGateArgs ga;
    if constexpr (GATE) ga = HubertGateArgs{p.gate_w, p.gate_b, p.gate_c, p.gates + (size_t)b * (p.F / kHubHeadDim) * p.T + t, (size_t)p.T};
    if constexpr (SPLIT) {
        char* const seq = reinterpret_cast<char*>(p.y + (size_t)b * p.Tout * p.F);
        hubert_ln_row<true, GATE>(v, lane, nv, p.F, p.eps, p.gamma, p.beta, GELU, nullptr,
                                  p.window ? hubert_window_ptr(seq, t, p.F) : seq + (size_t)t * p.F * 4, p.window ? 2 * p.F : p.F, &ga);
    } else {
        hubert_ln_row<false, GATE>(v, lane, nv, p.F, p.eps, p.gamma, p.beta, GELU, p.y + ((size_t)b * p.Tout + t) * p.F, nullptr, 0, &ga);
    }
}

// GELU in place on rows [B T][F] (F % 4 == 0); rows at or past a sequence's length are left alone.  grid (B T, ceil(F / 1024))
__global__ __launch_bounds__(256) void hubert_gelu_kernel(float* __restrict__ x, const int* __restrict__ lengths, int T, int F) {
    const long long row = blockIdx.x;
    const int b = (int)(row / T), t = (int)(row - (long long)b * T);
    const int len = lengths ? min(max(lengths[b], 0), T) : T;
    const int i = blockIdx.y * 256 + threadIdx.x;
    if (t >= len || 4 * i >= F) return;
    float4* const px = reinterpret_cast<float4*>(x + (size_t)row * F) + i;
    const float4 v = *px;
    *px = make_float4(hubert_gelu(v.x), hubert_gelu(v.y), hubert_gelu(v.z), hubert_gelu(v.w));
}

// The bf16x3 forward's GELU pass: rows [B T][F] fp32 -> the same rows, in place, as split rows [hi: F bf16 | lo: F bf16] of GELU(x), the
// operand of output_dense.  A split row's lo half lands where the row's second half of inputs lies, so ONE workgroup owns a row: it holds
// the row in registers (F <= 8192: eight float4 per thread) and stores behind a barrier.  F % 8 == 0 (threads i and i ^ 1 hold eight adjacent
// channels).  Rows at or past a sequence's length are left alone (the whole workgroup returns before the barrier).  grid (B T)
__global__ __launch_bounds__(256) void hubert_gelu_split_kernel(float* x, const int* __restrict__ lengths, int T, int F) {
    const long long row = blockIdx.x;
    const int b = (int)(row / T), t = (int)(row - (long long)b * T);
    const int len = lengths ? min(max(lengths[b], 0), T) : T;
    if (t >= len) return;
    const int nv = F >> 2;
    const float4* const px = reinterpret_cast<const float4*>(x + (size_t)row * F);
    float4 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int i = threadIdx.x + 256 * j;
        v[j] = i < nv ? px[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    char* const ys = reinterpret_cast<char*>(x) + (size_t)row * F * 4;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int i = threadIdx.x + 256 * j;
        if (i >= nv) continue;  // (nv is even: threads i and i ^ 1 pass together)
        xfmr_store_split(ys, F, 4 * i, i & 1, 1, hubert_gelu(v[j].x), hubert_gelu(v[j].y), hubert_gelu(v[j].z), hubert_gelu(v[j].w), true);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The positional conv: Conv1d(H, H, 128, padding 64, groups 16) with its last output frame dropped, + bias, GELU, added to the stream:
//     y[t, o] = x[t, o] + GELU(b[o] + sum_{k < 128} sum_{c < G} W[o, c, k] x[t + k - 64, grp G + c]),   frames outside 0 .. len - 1 are zeros.
// One workgroup per (sequence, group, tile of 128 frames).  The tile's rows and its halo (64 before, 63 behind) of the group's G channels are
// staged in LDS once; the taps are walked in order, each a G x G product per 16-frame block on v_mfma_f32_16x16x4_f32, computed transposed:
// the A operand is the weight block (16 output channels x 4 input channels), the B operand 4 input channels x 16 frames read from LDS at the
// tap's row offset, so a lane's four accumulator registers are four adjacent output channels of one frame: one float4 store.  Wave w owns
// frames 32 w .. 32 w + 31 of the tile and all the group's output channels.  The weights are read from global memory in MFMA lane order
// (wp: [group][tap][NOB][G / 4][64 lanes], output channels past G zeros; folded from weight_g / weight_v at hand-over): every wave of
// every tile of a group streams the same 128 G G floats, which stay in L2.  An output's sum runs over (tap, input channel) in one fixed order.
// pos_out (debug tap, or null): GELU(conv + b) alone.  y must not be x.
// ---------------------------------------------------------------------------------------------------------------------------
struct HubertPosParams {
    const float* x;        // [B T][H]
    const float* wp;
    const float* bias;     // [H]
    const int* lengths;    // frames, device, or null
    float* y;              // [B T][H]
    float* pos_out;        // [B T][H] or null
    int T, H;
};

template <int G>
struct HubertPosLds {
    static constexpr int pitch = G + 4;
    static constexpr int rows = kHubPosTR + kHubPosTaps - 1;
    static constexpr size_t bytes = (size_t)rows * pitch * sizeof(float);
};

template <int G>
__global__ __launch_bounds__(256) void hubert_posconv_kernel(const HubertPosParams p) {
    extern __shared__ float hubert_lds[];
    constexpr int PT = HubertPosLds<G>::pitch, NR = HubertPosLds<G>::rows, V = G / 4, NOB = (G + 15) / 16, NS = G / 4, NT = 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int b = blockIdx.z, grp = blockIdx.y, t0 = blockIdx.x * kHubPosTR;
    const int len = p.lengths ? min(max(p.lengths[b], 0), p.T) : p.T;
    if (t0 >= len) return;  // (the whole workgroup, before any barrier)
    const size_t row0 = (size_t)b * p.T;
    for (int i = tid; i < NR * V; i += 256) {
        const int r = i / V, v = i - r * V;
        const int t = t0 - kHubPosTaps / 2 + r;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t >= 0 && t < len) x = *reinterpret_cast<const float4*>(p.x + (row0 + t) * p.H + grp * G + 4 * v);
        *reinterpret_cast<float4*>(hubert_lds + r * PT + 4 * v) = x;
    }
    __syncthreads();
    if (t0 + wave * 32 >= len) return;  // (no barrier behind this point)

    f32x4 acc[NT][NOB];
#pragma unroll
    for (int tb = 0; tb < NT; ++tb)
#pragma unroll
        for (int ob = 0; ob < NOB; ++ob) acc[tb][ob] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* const wg = p.wp + (size_t)grp * kHubPosTaps * NOB * NS * 64 + lane;
    const float* const xw = hubert_lds + (wave * 32 + c) * PT + g;
    for (int k = 0; k < kHubPosTaps; ++k) {
        const float* const wk = wg + (size_t)k * NOB * NS * 64;
        const float* const xk = xw + k * PT;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            float bx[NT];
#pragma unroll
            for (int tb = 0; tb < NT; ++tb) bx[tb] = xk[tb * 16 * PT + 4 * s];
#pragma unroll
            for (int ob = 0; ob < NOB; ++ob) {
                const float a = wk[(ob * NS + s) * 64];
#pragma unroll
                for (int tb = 0; tb < NT; ++tb) acc[tb][ob] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bx[tb], acc[tb][ob], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int tb = 0; tb < NT; ++tb) {
        const int tl = wave * 32 + tb * 16 + c, t = t0 + tl;
        if (t >= len) continue;
#pragma unroll
        for (int ob = 0; ob < NOB; ++ob) {
            const int o = ob * 16 + 4 * g;  // this lane's four output channels of the group
            if (o >= G) continue;
            const float4 bv = *reinterpret_cast<const float4*>(p.bias + grp * G + o);
            const float4 xr = *reinterpret_cast<const float4*>(hubert_lds + (tl + kHubPosTaps / 2) * PT + o);
            const float4 e = make_float4(hubert_gelu(acc[tb][ob][0] + bv.x), hubert_gelu(acc[tb][ob][1] + bv.y), hubert_gelu(acc[tb][ob][2] + bv.z),
                                         hubert_gelu(acc[tb][ob][3] + bv.w));
            const size_t at = (row0 + t) * p.H + grp * G + o;
            *reinterpret_cast<float4*>(p.y + at) = make_float4(xr.x + e.x, xr.y + e.y, xr.z + e.z, xr.w + e.w);
            if (p.pos_out) *reinterpret_cast<float4*>(p.pos_out + at) = e;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Full softmax attention of one head over the utterance's own keys: S[q, k] = (Q[q] . K[k]) / sqrt(d), k < len.  xfmr_attn_kernel's plan — one
// workgroup per (sequence, head, tile of 64 queries), wave w owns queries 16 w .. 16 w + 15, everything computed transposed on
// v_mfma_f32_16x16x4_f32 so that a query is a lane column, online softmax per 64-key block, P never in LDS — without band, table or positional
// LDS region.  Keys past the length are skipped by predicate (weight 0, no part in the maximum); queries past it are not computed, their rows
// of `out` not written.  The head count is the grid's y extent.  The order of every sum depends on the sequence's length only.
// SPLIT (the bf16x3 forward): `out` is out_proj's input and nothing else, so the rows are stored as split rows only (out: [B T][4 F bytes]),
// as xfmr_attn_kernel<D, false, true> stores them.
// RELBIAS (WavLM): S[q, k] += gate[b, h, q] bias[h][clamp(k - q, -maxd, maxd) + maxd] in fp32, behind the scaling and in front of the running
// maximum.  A lane loads its query's gate once.  Per key block the workgroup stages, between the barriers that fence the K and V tiles, the
// 127 entries of the head's table that the block's 64 x 64 (key, query) pairs can meet: rel[j] = bias[h][clamp(kb - q0 - 63 + j)], so key
// kb + kk against query q0 + ql reads rel[kk - ql + 63].  512 bytes of LDS behind the V tile.  Banks: a wave's ds_read_b32 for register i of
// key block sb reads index 16 sb + 4 g + i - 16 w - c + 63 — within a 32-lane half (two values of g, sixteen of c) 20 consecutive dwords, equal
// indices the same address (broadcast): conflict-free in both directions.
// ---------------------------------------------------------------------------------------------------------------------------
struct HubertAttnParams {
    const float* qkv;    // [B T][3 F]: q | k | v, each [head][d]
    const int* lengths;  // device, or null
    float* out;          // [B T][F]: [head][d]
    int T, F;
    float scale;         // 1 / sqrt(d)
    const float* gates = nullptr;  // RELBIAS: (B, heads, T)
    const float* bias = nullptr;   //          [heads][2 maxd + 1]
    int maxd = 0;
};

constexpr int kHubRelSlice = 2 * kXfmrKB;  // 127 entries used

template <int D, bool RELBIAS = false>
struct HubertAttnLds {
    static constexpr size_t bytes = ((size_t)2 * kXfmrKB * (D + 4) + (RELBIAS ? kHubRelSlice : 0)) * sizeof(float);
};

template <int D, bool SPLIT = false, bool RELBIAS = false>
__global__ __launch_bounds__(256) void hubert_attn_kernel(const HubertAttnParams p) {
    static_assert(kXfmrKB == 64 && kXfmrTQ == 64, "the relative-bias slice is laid out for 64 keys x 64 queries");
    extern __shared__ float hubert_lds[];
    constexpr int PT = D + 4, NS = D / 4, NM = D / 16;
    float* const kbuf = hubert_lds;
    float* const vbuf = hubert_lds + kXfmrKB * PT;
    float* const rel = hubert_lds + 2 * kXfmrKB * PT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * kXfmrTQ;
    const int len = p.lengths ? min(max(p.lengths[b], 0), p.T) : p.T;
    if (q0 >= len) return;  // (the whole workgroup: no barrier has been reached)
    const size_t row0 = (size_t)b * p.T;
    const size_t F3 = (size_t)3 * p.F;
    const int q = q0 + wave * 16 + c;
    const bool qok = q < len;

    float qf[NS];  // this lane's B operands: Q[q][4 s + g]
    {
        const float* qrow = p.qkv + (row0 + (qok ? q : q0)) * F3 + h * D;
#pragma unroll
        for (int s = 0; s < NS; ++s) qf[s] = qok ? qrow[4 * s + g] : 0.f;
    }
    float gq = 0.f;  // this lane's query's gate
    const float* relq = rel;
    if constexpr (RELBIAS) {
        if (qok) gq = p.gates[((size_t)b * gridDim.y + h) * p.T + q];
        relq = rel + 63 - (wave * 16 + c) + 4 * g;  // + 16 sb + i: 0 .. 126
    }
    float m = -INFINITY, l = 0.f;
    f32x4 o[NM];
#pragma unroll
    for (int j = 0; j < NM; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int kb = 0; kb < len; kb += kXfmrKB) {
        const int n = min(kXfmrKB, len - kb);
        __syncthreads();
        xfmr_stage<D>(kbuf, p.qkv + (row0 + kb) * F3 + p.F + h * D, F3, n, tid);
        xfmr_stage<D>(vbuf, p.qkv + (row0 + kb) * F3 + 2 * p.F + h * D, F3, n, tid);
        if constexpr (RELBIAS) {
            if (tid < kHubRelSlice - 1)
                rel[tid] = p.bias[(size_t)h * (2 * p.maxd + 1) + (min(max(kb - q0 - 63 + tid, -p.maxd), p.maxd) + p.maxd)];
        }
        __syncthreads();

        f32x4 s[4];
        unsigned valid = 0;  // bit 4 sb + i: key kb + 16 sb + 4 g + i exists
        float mb = -INFINITY;
#pragma unroll
        for (int sb = 0; sb < 4; ++sb) {
            s[sb] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (16 * sb >= n) continue;  // (workgroup-uniform)
            const float* a = kbuf + (16 * sb + c) * PT + g;
#pragma unroll
            for (int st = 0; st < NS; ++st) s[sb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * st], qf[st], s[sb], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (qok && 16 * sb + 4 * g + i < n) {
                    float v = s[sb][i] * p.scale;
                    if constexpr (RELBIAS) v += gq * relq[16 * sb + i];
                    s[sb][i] = v;
                    mb = fmaxf(mb, v);
                    valid |= 1u << (4 * sb + i);
                }
            }
        }
        mb = fmaxf(mb, __shfl_xor(mb, 16));
        mb = fmaxf(mb, __shfl_xor(mb, 32));
        const float m_new = fmaxf(m, mb);
        const float alpha = m_new == -INFINITY ? 1.f : expf(m - m_new);
        float ls = 0.f;
#pragma unroll
        for (int sb = 0; sb < 4; ++sb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float e = (valid >> (4 * sb + i)) & 1u ? expf(s[sb][i] - m_new) : 0.f;
                s[sb][i] = e;
                ls += e;
            }
        ls += __shfl_xor(ls, 16);
        ls += __shfl_xor(ls, 32);
        l = l * alpha + ls;
        m = m_new;
#pragma unroll
        for (int j = 0; j < NM; ++j) o[j] *= alpha;
#pragma unroll
        for (int sb = 0; sb < 4; ++sb) {
            if (16 * sb >= n) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float* a = vbuf + (16 * sb + 4 * g + i) * PT + c;
#pragma unroll
                for (int j = 0; j < NM; ++j) o[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[16 * j], s[sb][i], o[j], 0, 0, 0);
            }
        }
    }
    if constexpr (SPLIT) {
        const float inv = qok ? 1.f / l : 0.f;
        char* const orow = reinterpret_cast<char*>(p.out) + (row0 + (qok ? q : q0)) * (size_t)p.F * 4;  // (qok is shared by the lanes of a column)
#pragma unroll
        for (int j = 0; j < NM; ++j)
            xfmr_store_split(orow, p.F, h * D + 16 * j + 4 * g, g & 1, 16, o[j][0] * inv, o[j][1] * inv, o[j][2] * inv, o[j][3] * inv, qok);
        return;
    }
    if (!qok) return;
    const float inv = 1.f / l;  // (l >= 1: the query's own key exists)
    float* orow = p.out + (row0 + q) * p.F + h * D + 4 * g;
#pragma unroll
    for (int j = 0; j < NM; ++j)
        *reinterpret_cast<float4*>(orow + 16 * j) = make_float4(o[j][0] * inv, o[j][1] * inv, o[j][2] * inv, o[j][3] * inv);
}

}  // namespace hificar
