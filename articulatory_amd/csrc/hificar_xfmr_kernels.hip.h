// Kernels of the Transformer feature model (articulatory/models/transformer.py:21-105, layers articulatory/layers/pytorch_layers.py:94-423)
// that are not GEMMs: the banded relative-position attention, the post-LayerNorm, and the layout changes at both ends.  Exact fp32
// arithmetic throughout; the bf16x3 forward's variants (xfmr_rows_split_kernel, xfmr_ln_kernel<true>, xfmr_attn_kernel<D, false, true>) differ
// in the FORMAT they store — split rows for the bf16x3 GEMM that reads them (xfmr_store_split) — not in how they compute.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hificar_conv.hip.h"
#include "hificar_bigru_train_kernels.hip.h"

namespace hificar {

constexpr int kXfmrHeads = 8;                // nhead of the reference's TransformerEncoderLayer (transformer.py:43)
constexpr int kXfmrRel = 100;                // relative_positional_distance
constexpr int kXfmrTab = 2 * kXfmrRel - 1;   // rows of one head's table: relative positions -99 .. 99
constexpr int kXfmrFF = 3072;                // dim_feedforward
constexpr int kXfmrTQ = 64;                  // queries per workgroup: four waves of 16
constexpr int kXfmrKB = 64;                  // keys per staged block
constexpr int kXfmrPosPitch = 211;           // floats per query row of the positional logits in LDS (2-way bank conflicts on the skewed read)

// ---------------------------------------------------------------------------------------------------------------------------
// Banded attention with learned relative positions (MultiHeadAttention.forward, pytorch_layers.py:205-229, with
// LearnedRelativePositionalEmbedding :280-423).  For a sequence of more than 100 frames the reference subtracts 1e8 from every logit with
// |k - q| >= 100, which is weight exactly 0 in fp32; for a shorter one the table index is the same formula.  So, per head,
//     S[q, k] = (Q[q] . K[k]) / sqrt(d) + Q[q] . E[k - q + 99]     for |k - q| <= 99, 0 <= k < length,     softmax over those keys only.
// Keys outside the band or past the sequence's length are skipped (a per-element predicate: weight 0, no part in the maximum), never
// masked with a large number.
//
// One workgroup per (sequence, head, tile of 64 queries); wave w owns queries 16 w .. 16 w + 15 of the tile.  Everything is computed
// TRANSPOSED with v_mfma_f32_16x16x4_f32, so that a query is a lane column (lane & 15) from start to end:
//   P^T = E Q^T   (199 x 16)  once, through LDS (pos[query][r]): the skew r = k - q + 99 is a per-lane address afterwards
//   S^T = K Q^T   (16 keys x 16 queries per step): lane holds keys 4 (lane >> 4) + i, i = 0 .. 3, of its query
//   O^T += V^T P^T: the accumulator registers of S^T ARE the B operands (register i = keys {4 g + i}: the A operand reads V rows in that order)
// so the softmax statistics are per lane (two xor-shuffles join the four lane groups of a column) and P never goes through LDS.
// K and V rows of the tile's band are staged in LDS in blocks of 64 keys (E in the same buffer before them); a wave skips the 16-key steps
// outside its own queries' band.  Online softmax per 64-key block.  The order of every sum depends on the query's position and the sequence's
// length only.
// ---------------------------------------------------------------------------------------------------------------------------
struct XfmrAttnParams {
    const float* qkv;    // [B T][3 F]: q | k | v, each [head][d]
    const float* emb;    // [8][199][d]
    const int* lengths;  // device, or null
    float* out;          // [B T][F]: [head][d]
    int T, F;
    float scale;         // 1 / sqrt(d)
    // the training instantiation only (hificar_xfmr_train_kernels.hip.h)
    float* lse = nullptr;                   // [B][8][T]: m + log l of every query's softmax
    const BigruTapeHeader* hdr = nullptr;   // seed, offset and p of the dropout on the probabilities
    int site = 0;
    const int* row0 = nullptr;              // [B + 1]: the packed layout (sequence b's rows start at row0[b]; lse is [rows][8]); null: b T
};

// Dropout of the Transformer's training step: the BiGRU's generator (BigruDrop: splitmix64 of key + element, top 24 bits against p) with a
// key that has room for the encoder's sites, key = mix(seed ^ mix(128 offset + site)); site 4 l + {0: attention probabilities, 1: dropout1,
// 2: the feed-forward's hidden rows, 3: dropout2}.  Element: the row-major index in (B, T, C); site 0: ((b 8 + h) T + q) 199 + (k - q + 99).
// The numpy restatement is articulatory_amd.utils.synth.xfmr_dropout_mask.
struct XfmrDrop {
    unsigned long long key;
    float p, scale;
    __device__ __forceinline__ XfmrDrop(const BigruTapeHeader* hdr, int site) {
        p = hdr->p;
        scale = p > 0.f ? 1.f / (1.f - p) : 1.f;
        key = bigru_mix64(hdr->seed ^ bigru_mix64(hdr->offset * 128ull + (unsigned long long)site));
    }
    __device__ __forceinline__ float operator()(unsigned long long e) const {
        if (!(p > 0.f)) return 1.f;
        const float u = (float)(unsigned)(bigru_mix64(key + e) >> 40) * (1.f / 16777216.f);
        return u >= p ? scale : 0.f;
    }
};

template <int D>
struct XfmrAttnLds {
    static constexpr int pitch = D + 4;  // (D / 4 + 1 is odd: the 16 rows x 4 columns a wave reads per MFMA operand fall in 64 different banks)
    static constexpr size_t bytes = ((size_t)2 * kXfmrKB * pitch + (size_t)kXfmrTQ * kXfmrPosPitch) * sizeof(float);
};

// rows [0, n) of a [..][stride] matrix (D floats each) -> dst[64][D + 4]; rows n .. 63 are zeros
template <int D>
__device__ __forceinline__ void xfmr_stage(float* dst, const float* src, size_t stride, int n, int tid) {
    constexpr int V = D / 4, PT = D + 4;
    for (int i = tid; i < kXfmrKB * V; i += 256) {
        const int r = i / V, v = i - r * V;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < n) x = *reinterpret_cast<const float4*>(src + (size_t)r * stride + 4 * v);
        *reinterpret_cast<float4*>(dst + r * PT + 4 * v) = x;
    }
}

// lane (c, g)'s share of one head's D floats of a row, as the attention kernels write it (columns 16 j + 4 g .. + 3), as zeros: the rows of
// padded frames (q < T at or past the sequence's length), which the GEMMs over all B T rows read
template <int D>
__device__ __forceinline__ void xfmr_zero_head_row(float* row4g, bool in_tensor) {
    if (!in_tensor) return;
#pragma unroll
    for (int j = 0; j < D / 16; ++j) *reinterpret_cast<float4*>(row4g + 16 * j) = make_float4(0.f, 0.f, 0.f, 0.f);
}

// The bf16x3 GEMMs' input format ("split rows", hificar_conv.hip.h): per row [hi: F bf16 | lo: F bf16], hi = bf16(x), lo = bf16(x - hi) — the
// expression of the conv engine's own output pass, so a consumer cannot tell its producers apart.  This lane holds channels ch4 .. ch4 + 3 of
// a row and lane ^ xm the neighbouring four (`odd`: this lane's are the upper four of the eight); the pair trades halves, so that the even
// lane stores 16 bytes of the hi half and the odd lane 16 bytes of the lo half.  Both lanes of a pair must be active; `store` is the same for both.
__device__ __forceinline__ void xfmr_store_split(char* row, int F, int ch4, bool odd, int xm, float a0, float a1, float a2, float a3, bool store) {
    const float a[4] = {a0, a1, a2, a3};
    bf16x4 hi, lo;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        hi[e] = (__bf16)a[e];
        lo[e] = (__bf16)(a[e] - (float)hi[e]);
    }
    const uint2 H = __builtin_bit_cast(uint2, hi), L = __builtin_bit_cast(uint2, lo);
    const uint2 send = odd ? H : L;
    const unsigned g0 = (unsigned)__shfl_xor((int)send.x, xm), g1 = (unsigned)__shfl_xor((int)send.y, xm);
    const uint4 pk = odd ? make_uint4(g0, g1, L.x, L.y) : make_uint4(H.x, H.y, g0, g1);
    if (store) *reinterpret_cast<uint4*>(row + (odd ? 2 * F : 0) + 2 * (odd ? ch4 - 4 : ch4)) = pk;
}

// TRAIN (the training forward): the kept probabilities are scaled by the dropout factor before P V (the denominator sums all of them, as
// F.softmax followed by nn.Dropout does), L = m + log l is kept per query, and the `out` rows of padded frames are written as zeros (a
// workgroup whose 64 queries are all padded writes them and returns).  The eval instantiation compiles none of it.
// first row of sequence b: b T, or the packed layout's table (training only)
template <bool TRAIN>
__device__ __forceinline__ size_t xfmr_attn_row0(const XfmrAttnParams& p, int b) {
    if constexpr (TRAIN) {
        if (p.row0) return (size_t)p.row0[b];
    }
    return (size_t)b * p.T;
}

// SPLIT (the bf16x3 forward; eval only): `out` is w_o's input and nothing else, so the rows are stored as split rows only (p.out: [B T][4 F
// bytes]).  Lanes g and g ^ 1 of a query column hold eight adjacent channels of every 16-channel block: xfmr_store_split, no pass through LDS.
template <int D, bool TRAIN = false, bool SPLIT = false>
__global__ __launch_bounds__(256) void xfmr_attn_kernel(const XfmrAttnParams p) {
    extern __shared__ float xfmr_lds[];
    constexpr int PT = D + 4, NS = D / 4, NM = D / 16, PP = kXfmrPosPitch;
    float* const kbuf = xfmr_lds;
    float* const vbuf = xfmr_lds + kXfmrKB * PT;
    float* const pos = xfmr_lds + 2 * kXfmrKB * PT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * kXfmrTQ;
    const int len = p.lengths ? min(max(p.lengths[b], 0), p.T) : p.T;
    const size_t row0 = xfmr_attn_row0<TRAIN>(p, b);
    const size_t F3 = (size_t)3 * p.F;
    const int qw = q0 + wave * 16, q = qw + c;
    const bool qok = q < len;
    if (q0 >= len) {  // (the whole workgroup: no barrier has been reached, nothing staged)
        // (packed: the rows past a length are another sequence's; the gap rows are xfmr_zero_gaps_kernel's)
        if constexpr (TRAIN) xfmr_zero_head_row<D>(p.out + (row0 + q) * p.F + h * D + 4 * g, q < p.T && !p.row0);
        return;
    }

    // this lane's B operands of every product: Q[q][4 s + g]
    float qf[NS];
    {
        const float* qrow = p.qkv + (row0 + (qok ? q : q0)) * F3 + h * D;
#pragma unroll
        for (int s = 0; s < NS; ++s) qf[s] = qok ? qrow[4 * s + g] : 0.f;
    }

    // positional logits of the wave's 16 queries: pos[16 wave + c][r] = Q[q] . E[r]
    float* const mypos = pos + (wave * 16 + c) * PP;
    for (int r0 = 0; r0 < kXfmrTab; r0 += kXfmrKB) {
        __syncthreads();
        xfmr_stage<D>(kbuf, p.emb + ((size_t)h * kXfmrTab + r0) * D, D, min(kXfmrKB, kXfmrTab - r0), tid);
        __syncthreads();
#pragma unroll
        for (int sb = 0; sb < 4; ++sb) {
            if (r0 + 16 * sb >= kXfmrTab) continue;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const float* a = kbuf + (16 * sb + c) * PT + g;
#pragma unroll
            for (int s = 0; s < NS; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * s], qf[s], acc, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = r0 + 16 * sb + 4 * g + i;
                if (r < kXfmrTab) mypos[r] = acc[i];
            }
        }
    }

    float m = -INFINITY, l = 0.f;  // running maximum (-inf: no key yet) and denominator of this lane's query
    f32x4 o[NM];
#pragma unroll
    for (int j = 0; j < NM; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int k_lo = max(0, q0 - (kXfmrRel - 1));
    const int k_hi = min(len, q0 + kXfmrTQ + (kXfmrRel - 1));
    for (int kb = k_lo; kb < k_hi; kb += kXfmrKB) {
        const int n = min(kXfmrKB, k_hi - kb);
        __syncthreads();
        xfmr_stage<D>(kbuf, p.qkv + (row0 + kb) * F3 + p.F + h * D, F3, n, tid);
        xfmr_stage<D>(vbuf, p.qkv + (row0 + kb) * F3 + 2 * p.F + h * D, F3, n, tid);
        __syncthreads();

        f32x4 s[4];
        unsigned valid = 0;  // bit 4 sb + i: key kb + 16 sb + 4 g + i is in this query's band and inside the sequence
        bool act[4];
        float mb = -INFINITY;
#pragma unroll
        for (int sb = 0; sb < 4; ++sb) {
            const int kk = kb + 16 * sb;
            // (wave-uniform) this 16-key step meets the band of the wave's queries qw .. qw + 15
            act[sb] = 16 * sb < n && kk + 15 >= qw - (kXfmrRel - 1) && kk <= qw + 15 + (kXfmrRel - 1);
            s[sb] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (!act[sb]) continue;
            const float* a = kbuf + (16 * sb + c) * PT + g;
#pragma unroll
            for (int st = 0; st < NS; ++st) s[sb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * st], qf[st], s[sb], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = kk + 4 * g + i;
                const int rel = k - q + (kXfmrRel - 1);
                const bool ok = qok && k < kb + n && rel >= 0 && rel < kXfmrTab;
                if (ok) {
                    const float v = s[sb][i] * p.scale + mypos[rel];
                    s[sb][i] = v;
                    mb = fmaxf(mb, v);
                    valid |= 1u << (4 * sb + i);
                }
            }
        }
        mb = fmaxf(mb, __shfl_xor(mb, 16));
        mb = fmaxf(mb, __shfl_xor(mb, 32));
        const float m_new = fmaxf(m, mb);
        const float alpha = m_new == -INFINITY ? 1.f : expf(m - m_new);  // (m = -inf, m_new finite: 0)
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
        if constexpr (TRAIN) {
            const XfmrDrop drop(p.hdr, p.site);
            const unsigned long long e0 = ((unsigned long long)(b * kXfmrHeads + h) * p.T + (qok ? q : 0)) * kXfmrTab;
#pragma unroll
            for (int sb = 0; sb < 4; ++sb)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if ((valid >> (4 * sb + i)) & 1u) s[sb][i] *= drop(e0 + (unsigned long long)(kb + 16 * sb + 4 * g + i - q + (kXfmrRel - 1)));
        }
#pragma unroll
        for (int j = 0; j < NM; ++j) o[j] *= alpha;
#pragma unroll
        for (int sb = 0; sb < 4; ++sb) {
            if (!act[sb]) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float* a = vbuf + (16 * sb + 4 * g + i) * PT + c;
#pragma unroll
                for (int j = 0; j < NM; ++j) o[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[16 * j], s[sb][i], o[j], 0, 0, 0);
            }
        }
    }
    if constexpr (SPLIT) {
        static_assert(!TRAIN, "split rows are an inference format");
        const float inv = qok ? 1.f / l : 0.f;
        char* const orow = reinterpret_cast<char*>(p.out) + (row0 + (qok ? q : q0)) * (size_t)p.F * 4;  // (qok is shared by the lanes of a column)
#pragma unroll
        for (int j = 0; j < NM; ++j)
            xfmr_store_split(orow, p.F, h * D + 16 * j + 4 * g, g & 1, 16, o[j][0] * inv, o[j][1] * inv, o[j][2] * inv, o[j][3] * inv, qok);
        return;
    }
    if (!qok) {
        // (training: w_o's GEMM and its weight gradient read every row of `out`; a padded frame's is zeros)
        if constexpr (TRAIN) xfmr_zero_head_row<D>(p.out + (row0 + q) * p.F + h * D + 4 * g, q < p.T && !p.row0);
        return;
    }
    const float inv = 1.f / l;  // (l >= 1: the query's own key is in its band)
    if constexpr (TRAIN) {
        if (g == 0) p.lse[p.row0 ? (row0 + q) * kXfmrHeads + h : ((size_t)b * kXfmrHeads + h) * p.T + q] = m + logf(l);
    }
    float* orow = p.out + (row0 + q) * p.F + h * D + 4 * g;
#pragma unroll
    for (int j = 0; j < NM; ++j)
        *reinterpret_cast<float4*>(orow + 16 * j) = make_float4(o[j][0] * inv, o[j][1] * inv, o[j][2] * inv, o[j][3] * inv);
}

// ---------------------------------------------------------------------------------------------------------------------------
// LayerNorm(F) (eps 1e-5, biased variance; torch.nn.LayerNorm, pytorch_layers.py:155-156): one wave per row, one pass over memory — the row
// lives in registers between the two reductions (mean, then squared deviations), whose lanes are joined in a fixed order.  F <= 1024, a
// multiple of 4.  Rows at or past a sequence's length are left alone (zero_pad: written as zeros).  x and y may be the same buffer.
// ---------------------------------------------------------------------------------------------------------------------------
struct XfmrLnParams {
    const float* x;
    const float* gamma;
    const float* beta;
    const int* lengths;  // device, or null
    float* y;
    int B, T, F;
    int zero_pad = 0;  // 1 (the ragged training step): rows at or past a length are written as zeros
    const int* pad_row = nullptr;  // the packed training step (B = 1, T = the packed rows, lengths null): a row r with pad_row[r] < 0 is a gap row
    char* ys = nullptr;  // xfmr_ln_kernel<true>: the same rows once more as split rows [B T][4 F bytes], the next GEMM's bf16x3 input
};

__device__ __forceinline__ float xfmr_wave_sum(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// SPLIT (the bf16x3 forward): the fp32 row (the next sub-block's residual) and its split copy p.ys (the next GEMM's input) in the same pass; F % 128 == 0
template <bool SPLIT = false>
__global__ __launch_bounds__(256) void xfmr_ln_kernel(const XfmrLnParams p) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long long)p.B * p.T) return;
    const int b = (int)(row / p.T), t = (int)(row - (long long)b * p.T);
    const int len = p.lengths ? min(max(p.lengths[b], 0), p.T) : p.T;
    const int nv = p.F >> 2;
    if (p.pad_row ? p.pad_row[row] < 0 : t >= len) {
        if (p.zero_pad)
            for (int i = lane; i < nv; i += 64) reinterpret_cast<float4*>(p.y + row * p.F)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const float4* x = reinterpret_cast<const float4*>(p.x + row * p.F);
    float4 v[4];
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = lane + 64 * j;
        v[j] = i < nv ? x[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        sum += (v[j].x + v[j].y) + (v[j].z + v[j].w);
    }
    const float mean = xfmr_wave_sum(sum) / (float)p.F;
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (lane + 64 * j >= nv) continue;
        const float a = v[j].x - mean, bb = v[j].y - mean, cc = v[j].z - mean, d = v[j].w - mean;
        sq += (a * a + bb * bb) + (cc * cc + d * d);
    }
    const float rstd = 1.f / sqrtf(xfmr_wave_sum(sq) / (float)p.F + 1e-5f);
    const float4* gm = reinterpret_cast<const float4*>(p.gamma);
    const float4* bt = reinterpret_cast<const float4*>(p.beta);
    float4* y = reinterpret_cast<float4*>(p.y + row * p.F);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = lane + 64 * j;
        if (i >= nv) continue;
        const float4 gv = gm[i], bv = bt[i];
        const float4 r = make_float4((v[j].x - mean) * rstd * gv.x + bv.x, (v[j].y - mean) * rstd * gv.y + bv.y, (v[j].z - mean) * rstd * gv.z + bv.z,
                                     (v[j].w - mean) * rstd * gv.w + bv.w);
        y[i] = r;
        // (F % 128 == 0, so nv is even: lanes i and i ^ 1 pass the test above together)
        if constexpr (SPLIT) xfmr_store_split(p.ys + row * p.F * 4, p.F, 4 * i, i & 1, 1, r.x, r.y, r.z, r.w, true);
    }
}

// x (B, C, T) fp32 -> rows [b T + t][Cp] (channels last; columns C .. Cp - 1 and frames at or past the sequence's length are zeros, the
// latter without being read).  row0 (the packed training step, null otherwise): rows [row0[b] + t], a sequence's own frames only
__global__ __launch_bounds__(256) void xfmr_rows_kernel(const float* __restrict__ x, float* __restrict__ rows, const int* __restrict__ lengths, int C,
                                                        int Cp, int T, const int* __restrict__ row0) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z, c0 = blockIdx.y * 32, t0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int len = lengths ? min(max(lengths[b], 0), T) : T;
    for (int r = ty; r < 32; r += 8) {
        const int c = c0 + r, t = t0 + tx;
        tile[r][tx] = (c < C && t < len) ? x[((size_t)b * C + c) * T + t] : 0.f;
    }
    __syncthreads();
    const size_t base = row0 ? (size_t)row0[b] : (size_t)b * T;
    const int tw = row0 ? len : T;
    for (int r = ty; r < 32; r += 8) {
        const int t = t0 + r, c = c0 + tx;
        if (t < tw && c < Cp) rows[(base + t) * Cp + c] = tile[tx][r];
    }
}

// The bf16x3 forward's input: the same rows as split rows [b T + t][hi: Cp bf16 | lo: Cp bf16] (raw: no activation; the padded channels are
// zero bits), one 16-byte store per thread: thread u writes eight channels of one half of row u / 8.  rows32 (non-null when in_channels ==
// hidden_dim: the input is block 0's fp32 residual as well as its operand): the fp32 rows too, as xfmr_rows_kernel writes them.
__global__ __launch_bounds__(256) void xfmr_rows_split_kernel(const float* __restrict__ x, char* __restrict__ rows, float* __restrict__ rows32,
                                                              const int* __restrict__ lengths, int C, int Cp, int T) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z, c0 = blockIdx.y * 32, t0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int len = lengths ? min(max(lengths[b], 0), T) : T;
    for (int r = ty; r < 32; r += 8) {
        const int c = c0 + r, t = t0 + tx;
        tile[r][tx] = (c < C && t < len) ? x[((size_t)b * C + c) * T + t] : 0.f;
    }
    __syncthreads();
    const size_t base = (size_t)b * T;
    if (rows32)
        for (int r = ty; r < 32; r += 8) {
            const int t = t0 + r, c = c0 + tx;
            if (t < T && c < Cp) rows32[(base + t) * Cp + c] = tile[tx][r];
        }
    const int r = threadIdx.x >> 3, half = (threadIdx.x >> 2) & 1, c8 = (threadIdx.x & 3) * 8;
    const int t = t0 + r;
    if (t >= T || c0 + c8 >= Cp) return;  // (32 | Cp)
    bf16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float a = tile[c8 + e][r];
        const __bf16 hi = (__bf16)a;
        v[e] = half ? (__bf16)(a - (float)hi) : hi;
    }
    *reinterpret_cast<bf16x8*>(rows + (base + t) * (size_t)Cp * 4 + (half ? 2 * Cp : 0) + 2 * (c0 + c8)) = v;
}

// rows [b T + t][Cp] -> out (B, C, T); frames at or past the sequence's length are written as zeros (their rows are not read)
// row0 (the packed training step, null otherwise): rows [row0[b] + t]
__global__ __launch_bounds__(256) void xfmr_out_kernel(const float* __restrict__ rows, float* __restrict__ out, const int* __restrict__ lengths, int C,
                                                       int Cp, int T, const int* __restrict__ row0) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z, c0 = blockIdx.y * 32, t0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int len = lengths ? min(max(lengths[b], 0), T) : T;
    const size_t base = row0 ? (size_t)row0[b] : (size_t)b * T;
    for (int r = ty; r < 32; r += 8) {
        const int t = t0 + r, c = c0 + tx;
        tile[r][tx] = (t < len && c < Cp) ? rows[(base + t) * Cp + c] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int c = c0 + r, t = t0 + tx;
        if (c < C && t < T) out[((size_t)b * C + c) * T + t] = tile[tx][r];
    }
}

}  // namespace hificar
