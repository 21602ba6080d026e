// Training kernels of the Transformer feature model (the reference's train() mode under autograd: articulatory/models/transformer.py:55-77,
// layers pytorch_layers.py:94-229): the backward of the banded relative-position attention, LayerNorm backwards, BatchNorm1d on batch
// statistics over conv rows, and the elementwise pieces (dropout, ReLU masks) between the GEMMs.  The GEMMs, their data gradients and their
// weight gradients run on the conv engine (hificar_xfmr_train.hip.inc).  Exact fp32; every reduction is summed in a fixed order (no atomics).
// Ragged batches (hificar_xfmr_forward_train_ragged): the tape keeps the frame counts (`lens`, honoured when its header says ragged).  The
// GEMMs run over all B T rows, so every kernel below that writes rows writes those of padded frames (at or past a sequence's count) as
// zeros without reading them, and every sum over rows skips them by a predicate — never by a multiplication (NaN * 0 is NaN).  A dense
// tape takes the same statements with every count = T.
// Packed batches (hificar_xfmr_forward_train_packed): the same rule over the rows of XfmrLayout, with a gap row where the ragged step has a
// padded frame's row; the kernels take the layout as an argument and execute the statements above when its tables are null.
#pragma once
#include "hificar_xfmr_kernels.hip.h"

namespace hificar {

constexpr int kXfmrBand = 200;      // floats per (b, h, q) row of the banded buffers: index k - q + 99 in 0 .. 198, one of padding
constexpr int kXfmrColRows = 256;   // rows per partial of the two-stage column sums
constexpr int kXfmrEmbRows = 256;   // rows per partial of the table gradient
constexpr int kXfmrEmbPitch = 208;  // floats per row of the staged dS block: 13 tiles of 16 table rows; 208 = 16 (mod 64): no bank conflicts

// The layout of a training step's rows.  Dense and ragged (both tables null): row b T + t is frame t of sequence b, and `lens` (null: dense)
// says which rows are padding.  Packed (hificar_xfmr_forward_train_packed): sequence b's frames are rows row0[b] .. row0[b] + lens[b] - 1,
// one gap row follows every sequence and the tail up to the row count is gap rows too; pad_row[r] is the padded index b T + t of packed
// row r, or -1 for a gap row.  A gap row is what a padded frame's row is to the ragged step: written as zeros, never read into a sum.
// The banded buffers and lse are [B][8][T] (dense, ragged) or [rows][8] (packed).
struct XfmrLayout {
    const int* row0 = nullptr;     // [B + 1]
    const int* pad_row = nullptr;  // [rows]
};

__device__ __forceinline__ bool xfmr_row_valid(const XfmrLayout& lay, const int* lens, long long r, int T) {
    if (lay.pad_row) return lay.pad_row[r] >= 0;
    return bigru_row_valid(lens, (int)r, T);
}
// element e of rows [rows][width] belongs to a frame of its sequence (dense: always)
__device__ __forceinline__ bool xfmr_elem_valid(const XfmrLayout& lay, const int* lens, long long e, int width, int T) {
    if (lay.pad_row) return lay.pad_row[e / width] >= 0;
    return !lens || bigru_row_valid(lens, (int)(e / width), T);
}
// the dropout element of element e of a valid row: its index in the PADDED (B, T, width) tensor (packed: through pad_row, in 64 bits)
__device__ __forceinline__ unsigned long long xfmr_drop_elem(const XfmrLayout& lay, long long e, int width) {
    if (!lay.pad_row) return (unsigned long long)e;
    const long long r = e / width;
    return (unsigned long long)((long long)lay.pad_row[r] * width + (e - r * width));
}
// first row of sequence b, and the index of (b, h, q) in lse and in the banded buffers' rows
__device__ __forceinline__ size_t xfmr_seq_row0(const XfmrLayout& lay, int b, int T) { return lay.row0 ? (size_t)lay.row0[b] : (size_t)b * T; }
__device__ __forceinline__ size_t xfmr_band_row(const XfmrLayout& lay, size_t row0, int b, int h, int q, int T) {
    return lay.row0 ? (row0 + q) * kXfmrHeads + h : ((size_t)b * kXfmrHeads + h) * T + q;
}

// pad_row and row0 of a packed forward from the frame counts.  grid (B + 1), block b: sequence b's rows and its gap row; block B: the tail.
// Writes stay below `rows` whatever the device counts hold (the host sized the tables from its own copy).
__global__ __launch_bounds__(256) void xfmr_pack_table_kernel(const int* __restrict__ lens, int B, int T, int rows, int* __restrict__ row0,
                                                              int* __restrict__ pad_row) {
    __shared__ int part[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    int s = 0;
    for (int i = tid; i < b; i += 256) s += min(max(lens[i], 0), T) + 1;
    part[tid] = s;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if (tid < d) part[tid] += part[tid + d];
        __syncthreads();
    }
    const int r0 = min(part[0], rows);
    if (tid == 0) row0[b] = r0;
    if (b == B) {
        for (int r = r0 + tid; r < rows; r += 256) pad_row[r] = -1;
        return;
    }
    const int len = min(max(lens[b], 0), T);
    for (int t = tid; t <= len; t += 256)
        if (r0 + t < rows) pad_row[r0 + t] = t < len ? b * T + t : -1;
}

// rows[r][0 .. width) = 0 for every gap row r (width % 4 == 0): the rows the layout kernels and the attention kernels of a packed step,
// which write a sequence's own rows only, leave to this one.  One wave per row.
__global__ __launch_bounds__(256) void xfmr_zero_gaps_kernel(float* __restrict__ rows, int width, const int* __restrict__ pad_row, int n) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n || pad_row[r] >= 0) return;
    for (int i = lane; i < width / 4; i += 64) reinterpret_cast<float4*>(rows + r * width)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// packed rows [row0[b] + t][width] -> dst (B, T, width), zeros on padded frames: the debug taps of a packed forward.  grid (blocks, B)
__global__ __launch_bounds__(256) void xfmr_unpack_rows_kernel(const float* __restrict__ rows, float* __restrict__ dst, int width,
                                                               const int* __restrict__ lens, const int* __restrict__ row0, int T) {
    const int b = blockIdx.y, w4 = width / 4;
    const long long n4 = (long long)T * w4, have = (long long)bigru_len(lens, b, T) * w4;
    const float4* const src = reinterpret_cast<const float4*>(rows + (size_t)row0[b] * width);
    float4* const out = reinterpret_cast<float4*>(dst + (size_t)b * T * width);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256)
        out[i] = i < have ? src[i] : make_float4(0.f, 0.f, 0.f, 0.f);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Attention backward.  With L = m + log l kept by the forward (XfmrAttnParams::lse), per head
//     P[q, k]  = exp(S[q, k] - L[q])                      recomputed exactly as the forward computed S
//     Pd       = P o mask / (1 - p)                       the probabilities the forward multiplied V with
//     Delta[q] = dO[q] . O[q]                             (= sum_k Pd dPd, since O = Pd V)
//     dS       = P o (dO V^T o mask / (1 - p) - Delta)
//     dQ[q]    = sum_k dS[q, k] (K[k] / sqrt(d) + E[k - q + 99])
//     dK[k]    = sum_q dS[q, k] Q[q] / sqrt(d),   dV[k] = sum_q Pd[q, k] dO[q],   dE[r] = sum_{b, q} dS[q, q + r - 99] Q[q]
// Keys outside the band or the sequence stay a predicate everywhere.  A ragged tape: the sequence's length is its frame count; the
// dq | dk | dv rows of padded frames are written as zeros (the fused q | k | v weight-gradient launch reads all rows), the banded dS and Pd
// rows of padded queries are neither written nor read, and a workgroup whose 64 queries (keys) are all padded stages nothing.
//
// The query-tiled kernel has xfmr_attn_kernel's layout (a query is a lane column): S^T = K Q^T and dPd^T = V dO^T are 16 x 16 tiles whose
// accumulator registers are the B operands of dQ^T += K^T dS^T.  dS of the wave's 16 queries replaces the positional logits in LDS entry by
// entry (each (q, r) is read once, by the lane that then writes it), so the positional part of dQ is one more product, E^T dS^T, over the
// 199 table rows, and the banded dS rows [B][8][T][200] go to memory from LDS in whole rows.  Pd goes to a second banded buffer.
// ---------------------------------------------------------------------------------------------------------------------------
struct XfmrAttnBwdParams {
    const float* qkv;   // [B T][3 F]
    const float* emb;   // [8][199][d]
    const float* o;     // [B T][F]: the forward's output rows
    const float* dout;  // [B T][F]
    const float* lse;   // [B][8][T]
    float* dqkv;        // [B T][3 F]: dq | dk | dv
    float* ds;          // [B][8][T][200]
    float* pd;          // [B][8][T][200]
    const BigruTapeHeader* hdr;
    const int* lens;    // [B]: the tape's frame counts (hdr->ragged)
    int site;
    int T, F;
    float scale;
    XfmrLayout lay;     // packed: rows [row0[b] + t], lse [rows][8], ds / pd [rows][8][200]
};

template <int D>
__global__ __launch_bounds__(256) void xfmr_attn_bwd_q_kernel(const XfmrAttnBwdParams p) {
    extern __shared__ float xfmr_lds[];
    constexpr int PT = D + 4, NS = D / 4, NM = D / 16, PP = kXfmrPosPitch;
    float* const kbuf = xfmr_lds;
    float* const vbuf = xfmr_lds + kXfmrKB * PT;
    float* const pos = xfmr_lds + 2 * kXfmrKB * PT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * kXfmrTQ;
    const int len = bigru_len(bigru_tape_lens(p.hdr, p.lens), b, p.T);
    const size_t row0 = xfmr_seq_row0(p.lay, b, p.T);
    const size_t F3 = (size_t)3 * p.F;
    const size_t bh = (size_t)b * kXfmrHeads + h;
    const int qw = q0 + wave * 16, q = qw + c;
    const bool qok = q < len;
    const bool zero_pad = !p.lay.row0;  // (packed: the rows past a length are another sequence's; the gap rows are xfmr_zero_gaps_kernel's)
    if (q0 >= len) {  // (the whole workgroup, before any barrier) 64 padded queries: their dq rows are zeros
        xfmr_zero_head_row<D>(p.dqkv + (row0 + q) * F3 + h * D + 4 * g, q < p.T && zero_pad);
        return;
    }
    const XfmrDrop drop(p.hdr, p.site);

    float qf[NS], dof[NS];
    float delta = 0.f, lq = 0.f;
    {
        const size_t r = row0 + (qok ? q : q0);
        const float* qrow = p.qkv + r * F3 + h * D;
        const float* drow = p.dout + r * p.F + h * D;
        const float* orow = p.o + r * p.F + h * D;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            qf[s] = qok ? qrow[4 * s + g] : 0.f;
            dof[s] = qok ? drow[4 * s + g] : 0.f;
            delta = fmaf(dof[s], qok ? orow[4 * s + g] : 0.f, delta);
        }
        delta += __shfl_xor(delta, 16);
        delta += __shfl_xor(delta, 32);
        if (qok) lq = p.lse[xfmr_band_row(p.lay, row0, b, h, q, p.T)];
    }

    // positional logits of the wave's 16 queries, as the forward: pos[16 wave + c][r] = Q[q] . E[r]
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

    f32x4 o[NM];  // dQ^T of this lane's query: rows 16 j + 4 g + i
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
#pragma unroll
        for (int sb = 0; sb < 4; ++sb) {
            const int kk = kb + 16 * sb;
            // (wave-uniform) this 16-key step meets the band of the wave's queries
            if (!(16 * sb < n && kk + 15 >= qw - (kXfmrRel - 1) && kk <= qw + 15 + (kXfmrRel - 1))) continue;
            f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
            const float* ak = kbuf + (16 * sb + c) * PT + g;
            const float* av = vbuf + (16 * sb + c) * PT + g;
#pragma unroll
            for (int st = 0; st < NS; ++st) s = __builtin_amdgcn_mfma_f32_16x16x4f32(ak[4 * st], qf[st], s, 0, 0, 0);
#pragma unroll
            for (int st = 0; st < NS; ++st) dp = __builtin_amdgcn_mfma_f32_16x16x4f32(av[4 * st], dof[st], dp, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = kk + 4 * g + i;
                const int rel = k - q + (kXfmrRel - 1);
                const bool ok = qok && k < kb + n && rel >= 0 && rel < kXfmrTab;
                float dsv = 0.f;
                if (ok) {
                    const float pr = expf(s[i] * p.scale + mypos[rel] - lq);
                    const float f = drop((bh * p.T + q) * kXfmrTab + rel);
                    dsv = pr * (dp[i] * f - delta);
                    mypos[rel] = dsv;
                    p.pd[xfmr_band_row(p.lay, row0, b, h, q, p.T) * kXfmrBand + rel] = pr * f;
                }
                s[i] = dsv;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float* a = kbuf + (16 * sb + 4 * g + i) * PT + c;
#pragma unroll
                for (int j = 0; j < NM; ++j) o[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[16 * j], s[i], o[j], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NM; ++j) o[j] *= p.scale;

    // The wave's 16 rows of dS: what no key visited (before the sequence's start, past its end, a query past the end) still holds a
    // positional logit: zero it; then the rows go to memory whole (entry 199 is padding, written as zero).
    for (int i = lane; i < 16 * kXfmrBand; i += 64) {
        const int qq = i / kXfmrBand, r = i - qq * kXfmrBand;
        const int qa = qw + qq, k = qa + r - (kXfmrRel - 1);
        float* const e = pos + (wave * 16 + qq) * PP + r;
        float v = 0.f;
        if (qa < len && r < kXfmrTab && k >= 0 && k < len) v = *e;
        *e = v;
        if (qa < len) p.ds[xfmr_band_row(p.lay, row0, b, h, qa, p.T) * kXfmrBand + r] = v;
    }

    // dQ^T += E^T dS^T over the table rows (A: E[r][16 j + c], B: dS[q = c][r], r = 4 g-th of each step)
    for (int r0 = 0; r0 < kXfmrTab; r0 += kXfmrKB) {
        __syncthreads();
        xfmr_stage<D>(kbuf, p.emb + ((size_t)h * kXfmrTab + r0) * D, D, min(kXfmrKB, kXfmrTab - r0), tid);
        __syncthreads();
#pragma unroll 4
        for (int st = 0; st < kXfmrKB / 4; ++st) {
            const int r = r0 + 4 * st + g;
            if (r0 + 4 * st >= kXfmrTab) break;  // (wave-uniform)
            const float bv = r < kXfmrBand ? mypos[r] : 0.f;  // (r = 199: the zero written above)
            const float* a = kbuf + (4 * st + g) * PT + c;
#pragma unroll
            for (int j = 0; j < NM; ++j) o[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[16 * j], bv, o[j], 0, 0, 0);
        }
    }
    float* orow = p.dqkv + (row0 + q) * F3 + h * D + 4 * g;
    if (!qok) {
        xfmr_zero_head_row<D>(orow, q < p.T && zero_pad);
        return;
    }
#pragma unroll
    for (int j = 0; j < NM; ++j) *reinterpret_cast<float4*>(orow + 16 * j) = make_float4(o[j][0], o[j][1], o[j][2], o[j][3]);
}

// The key-tiled kernel: one workgroup per (sequence, head, 64 keys), a key is a lane column, the queries within +-99 are walked in blocks
// of 64 whose dO and Q rows are staged in LDS.  dV^T += dO^T Pd and dK^T += Q^T dS, with Pd and dS read from the banded buffers (the 16 keys
// of a column group are 16 consecutive floats of a query's row).
template <int D>
struct XfmrAttnBwdKLds {
    static constexpr size_t bytes = (size_t)2 * kXfmrKB * (D + 4) * sizeof(float);
};

template <int D>
__global__ __launch_bounds__(256) void xfmr_attn_bwd_k_kernel(const XfmrAttnBwdParams p) {
    extern __shared__ float xfmr_lds[];
    constexpr int PT = D + 4, NM = D / 16;
    float* const dobuf = xfmr_lds;
    float* const qbuf = xfmr_lds + kXfmrKB * PT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int b = blockIdx.z, h = blockIdx.y, k0 = blockIdx.x * kXfmrKB;
    const int len = bigru_len(bigru_tape_lens(p.hdr, p.lens), b, p.T);
    const size_t row0 = xfmr_seq_row0(p.lay, b, p.T);
    const size_t F3 = (size_t)3 * p.F;
    const int kw = k0 + wave * 16, k = kw + c;
    const bool kok = k < len;
    float* const krow = p.dqkv + (row0 + k) * F3 + p.F + h * D + 4 * g;
    float* const vrow = krow + p.F;
    const bool zero_pad = !p.lay.row0;  // (as in the query-tiled kernel)
    if (k0 >= len) {  // (the whole workgroup, before any barrier) 64 padded keys: their dk | dv rows are zeros
        xfmr_zero_head_row<D>(krow, k < p.T && zero_pad);
        xfmr_zero_head_row<D>(vrow, k < p.T && zero_pad);
        return;
    }
    f32x4 dv[NM], dk[NM];
#pragma unroll
    for (int j = 0; j < NM; ++j) dv[j] = dk[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int q_lo = max(0, k0 - (kXfmrRel - 1));
    const int q_hi = min(len, k0 + kXfmrKB + (kXfmrRel - 1));
    for (int qb = q_lo; qb < q_hi; qb += kXfmrKB) {
        const int n = min(kXfmrKB, q_hi - qb);
        __syncthreads();
        xfmr_stage<D>(dobuf, p.dout + (row0 + qb) * p.F + h * D, (size_t)p.F, n, tid);
        xfmr_stage<D>(qbuf, p.qkv + (row0 + qb) * F3 + h * D, F3, n, tid);
        __syncthreads();
        for (int st = 0; st < kXfmrKB / 4; ++st) {
            const int qq = qb + 4 * st;
            // (wave-uniform) these four queries meet the band of the wave's keys
            if (4 * st >= n) break;
            if (qq + 3 < kw - (kXfmrRel - 1) || qq > kw + 15 + (kXfmrRel - 1)) continue;
            const int q = qq + g;
            const int rel = k - q + (kXfmrRel - 1);
            float pv = 0.f, sv = 0.f;
            if (kok && q < qb + n && rel >= 0 && rel < kXfmrTab) {
                const size_t e = xfmr_band_row(p.lay, row0, b, h, q, p.T) * kXfmrBand + rel;
                pv = p.pd[e];
                sv = p.ds[e];
            }
            const float* ad = dobuf + (4 * st + g) * PT + c;
            const float* aq = qbuf + (4 * st + g) * PT + c;
#pragma unroll
            for (int j = 0; j < NM; ++j) {
                dv[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ad[16 * j], pv, dv[j], 0, 0, 0);
                dk[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq[16 * j], sv, dk[j], 0, 0, 0);
            }
        }
    }
    if (!kok) {
        xfmr_zero_head_row<D>(krow, k < p.T && zero_pad);
        xfmr_zero_head_row<D>(vrow, k < p.T && zero_pad);
        return;
    }
#pragma unroll
    for (int j = 0; j < NM; ++j) {
        *reinterpret_cast<float4*>(krow + 16 * j) = make_float4(dk[j][0] * p.scale, dk[j][1] * p.scale, dk[j][2] * p.scale, dk[j][3] * p.scale);
        *reinterpret_cast<float4*>(vrow + 16 * j) = make_float4(dv[j][0], dv[j][1], dv[j][2], dv[j][3]);
    }
}

// Table gradient, first stage: partial[chunk][h][r][d] = sum over the chunk's 256 rows (b, q) of dS[b, h, q, r] Q[b, h, q], the rows taken
// in blocks of 64 in order.  grid (chunks, 8).  Wave w owns the table-row tiles w, w + 4, w + 8 (and 12: wave 0).  The second stage
// (bigru_colreduce_kernel) adds the chunks in order.  The rows are those of the padded batch; a padded frame's row is staged as zeros
// (both operands, neither read) and a block of 64 rows without a valid one is skipped.
template <int D>
struct XfmrEmbLds {
    static constexpr size_t bytes = (size_t)64 * (D + 4 + kXfmrEmbPitch) * sizeof(float);
};

template <int D>
__global__ __launch_bounds__(256) void xfmr_demb_partial_kernel(const float* __restrict__ qkv, const float* __restrict__ ds, float* __restrict__ partial,
                                                                int M, int T, int F, const BigruTapeHeader* hdr, const int* __restrict__ tape_lens,
                                                                const XfmrLayout lay) {
    extern __shared__ float xfmr_lds[];
    constexpr int PT = D + 4, NM = D / 16, DP = kXfmrEmbPitch;
    float* const qbuf = xfmr_lds;
    float* const dbuf = xfmr_lds + 64 * PT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int chunk = blockIdx.x, h = blockIdx.y;
    const size_t F3 = (size_t)3 * F;
    const int* const lens = bigru_tape_lens(hdr, tape_lens);
    f32x4 acc[4][NM];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int j = 0; j < NM; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int blk = 0; blk < kXfmrEmbRows / 64; ++blk) {
        const int r0 = chunk * kXfmrEmbRows + blk * 64;
        if (r0 >= M) break;  // (the whole workgroup)
        const int n = min(64, M - r0);
        if (lay.pad_row) {  // (the whole workgroup) packed rows: the same question asked of the table
            bool any = false;
            for (int i = 0; i < n; ++i) any = any || lay.pad_row[r0 + i] >= 0;
            if (!any) continue;
        } else if (lens) {  // (the whole workgroup) no frame among these rows: nothing to add
            bool any = false;
            for (int bb = r0 / T; bb <= (r0 + n - 1) / T; ++bb) any = any || max(r0, bb * T) < min(r0 + n, bb * T + bigru_len(lens, bb, T));
            if (!any) continue;
        }
        __syncthreads();
        if (!lens) {
            xfmr_stage<D>(qbuf, qkv + (size_t)r0 * F3 + h * D, F3, n, tid);
        } else {
            for (int i = tid; i < 64 * (D / 4); i += 256) {
                const int rr = i / (D / 4), v = i - rr * (D / 4);
                float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                if (rr < n && xfmr_row_valid(lay, lens, r0 + rr, T)) x = *reinterpret_cast<const float4*>(qkv + (size_t)(r0 + rr) * F3 + h * D + 4 * v);
                *reinterpret_cast<float4*>(qbuf + rr * PT + 4 * v) = x;
            }
        }
        for (int i = tid; i < 64 * (DP / 4); i += 256) {
            const int rr = i / (DP / 4), v = i - rr * (DP / 4);
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (rr < n && 4 * v < kXfmrBand && xfmr_row_valid(lay, lens, r0 + rr, T)) {  // (entry 199 of a row is a written zero)
                const int row = r0 + rr, bb = row / T, t = row - bb * T;
                const size_t band = lay.pad_row ? (size_t)row * kXfmrHeads + h : ((size_t)bb * kXfmrHeads + h) * T + t;
                x = *reinterpret_cast<const float4*>(ds + band * kXfmrBand + 4 * v);
            }
            *reinterpret_cast<float4*>(dbuf + rr * DP + 4 * v) = x;
        }
        __syncthreads();
        for (int st = 0; st < 16; ++st) {
            if (4 * st >= n) break;
            float bq[NM];
#pragma unroll
            for (int j = 0; j < NM; ++j) bq[j] = qbuf[(4 * st + g) * PT + 16 * j + c];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int rt = wave + 4 * t;
                if (rt >= DP / 16) continue;
                const float a = dbuf[(4 * st + g) * DP + 16 * rt + c];
#pragma unroll
                for (int j = 0; j < NM; ++j) acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bq[j], acc[t][j], 0, 0, 0);
            }
        }
    }
    float* const dst = partial + ((size_t)chunk * kXfmrHeads + h) * kXfmrTab * D;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int rt = wave + 4 * t;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = 16 * rt + 4 * g + i;
            if (rt >= DP / 16 || r >= kXfmrTab) continue;
#pragma unroll
            for (int j = 0; j < NM; ++j) dst[(size_t)r * D + 16 * j + c] = acc[t][j][i];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Column sums over rows [M][F] in two fixed-order stages.  First stage: grid (F / 64, chunks of 256 rows), thread (row lane ty = 0 .. 3,
// column tx): rows ty, ty + 4, ... of the chunk, then the four lanes in order -> partial[chunk][2][F].  Second stage: one thread per column
// adds the chunks in order (the finishing kernels below, or bigru_colreduce_kernel over [2 F] for a (d gamma | d beta) pair).
//   mode 0  s0 = x                                               BatchNorm mean
//   mode 1  s0 = (x - mean[c])^2                                 BatchNorm variance: the second pass, not E[x^2] - E[x]^2
//   mode 2  s0 = dy xhat, s1 = dy, xhat = (x - mean[c]) rstd[c]  BatchNorm backward (stats: mean | var | rstd)
//   mode 3  s0 = dy xhat, s1 = dy, xhat = (x - mean_r) rstd_r    LayerNorm backward (rowstats[r]: mean, rstd of row r)
// A ragged tape: the chunks are those of the padded row index and a valid row keeps its lane and its turn; a padded row is skipped, not
// read.  The BatchNorm means divide by the tape's M, the number of valid rows.
// ---------------------------------------------------------------------------------------------------------------------------
struct XfmrColParams {
    const float* x;
    const float* dy;
    const float* stats;     // [3][F]
    const float* rowstats;  // [M][2]
    float* partial;         // [chunks][2][F]
    const BigruTapeHeader* hdr;
    const int* lens;        // [B]: the tape's frame counts (hdr->ragged)
    int M, T, F, mode;      // M = B T: the rows of the padded batch (packed: the packed rows)
    XfmrLayout lay;
};

__global__ __launch_bounds__(256) void xfmr_colsum_kernel(const XfmrColParams p) {
    __shared__ float red[2][4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6, c = blockIdx.x * 64 + tx;
    const int r0 = blockIdx.y * kXfmrColRows, r1 = min(p.M, r0 + kXfmrColRows);
    float mean = 0.f, rstd = 0.f;
    if (p.mode == 1 || p.mode == 2) mean = p.stats[c];
    if (p.mode == 2) rstd = p.stats[2 * p.F + c];
    const int* const lens = bigru_tape_lens(p.hdr, p.lens);
    float s0 = 0.f, s1 = 0.f;
    for (int r = r0 + ty; r < r1; r += 4) {
        if (!xfmr_row_valid(p.lay, lens, r, p.T)) continue;
        const size_t e = (size_t)r * p.F + c;
        const float x = p.x[e];
        if (p.mode == 0) {
            s0 += x;
        } else if (p.mode == 1) {
            s0 = fmaf(x - mean, x - mean, s0);
        } else {
            if (p.mode == 3) {
                mean = p.rowstats[2 * (size_t)r];
                rstd = p.rowstats[2 * (size_t)r + 1];
            }
            const float dy = p.dy[e];
            s0 = fmaf(dy, (x - mean) * rstd, s0);
            s1 += dy;
        }
    }
    red[0][ty][tx] = s0;
    red[1][ty][tx] = s1;
    __syncthreads();
    if (ty < 2) {
        const float s = ((red[ty][0][tx] + red[ty][1][tx]) + red[ty][2][tx]) + red[ty][3][tx];
        p.partial[((size_t)blockIdx.y * 2 + ty) * p.F + c] = s;
    }
}

// stats[c] = mean of column c (the chunks' sums added in order, in double)
__global__ __launch_bounds__(256) void xfmr_bn_mean_kernel(const float* __restrict__ partial, int chunks, int F, const BigruTapeHeader* hdr,
                                                           float* __restrict__ stats) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= F) return;
    const int M = hdr->M;
    double s = 0.0;
    for (int i = 0; i < chunks; ++i) s += (double)partial[(size_t)i * 2 * F + c];
    stats[c] = (float)(s / M);
}

// stats: mean | biased variance | 1 / sqrt(var + 1e-5); batch_stats (mean | biased variance) goes back to the caller
__global__ __launch_bounds__(256) void xfmr_bn_var_kernel(const float* __restrict__ partial, int chunks, int F, const BigruTapeHeader* hdr,
                                                          float* __restrict__ stats, float* __restrict__ batch_stats) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= F) return;
    const int M = hdr->M;
    double s = 0.0;
    for (int i = 0; i < chunks; ++i) s += (double)partial[(size_t)i * 2 * F + c];
    const float var = (float)(s / M);
    stats[F + c] = var;
    stats[2 * F + c] = 1.f / sqrtf(var + 1e-5f);
    batch_stats[c] = stats[c];
    batch_stats[F + c] = var;
}

// out = (x - mean) rstd gamma + beta (+ res) (ReLU'd with relu != 0) over rows [B T][F]; n4 = B T F / 4.  lens (null: dense): the rows of
// padded frames are written as zeros
__global__ __launch_bounds__(256) void xfmr_bn_apply_kernel(const float* __restrict__ x, const float* __restrict__ stats, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ res, float* __restrict__ out,
                                                            long long n4, int F, int relu, const int* __restrict__ lens, int T, const XfmrLayout lay) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        if (!xfmr_elem_valid(lay, lens, i * 4, F, T)) {
            reinterpret_cast<float4*>(out)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        const int c = (int)((i * 4) % F);
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        const float4 mu = *reinterpret_cast<const float4*>(stats + c), rs = *reinterpret_cast<const float4*>(stats + 2 * F + c);
        const float4 gm = *reinterpret_cast<const float4*>(gamma + c), bt = *reinterpret_cast<const float4*>(beta + c);
        float4 y = make_float4((v.x - mu.x) * rs.x * gm.x + bt.x, (v.y - mu.y) * rs.y * gm.y + bt.y, (v.z - mu.z) * rs.z * gm.z + bt.z,
                               (v.w - mu.w) * rs.w * gm.w + bt.w);
        if (res) {
            const float4 r = reinterpret_cast<const float4*>(res)[i];
            y = make_float4(y.x + r.x, y.y + r.y, y.z + r.z, y.w + r.w);
        }
        if (relu) y = make_float4(fmaxf(y.x, 0.f), fmaxf(y.y, 0.f), fmaxf(y.z, 0.f), fmaxf(y.w, 0.f));
        reinterpret_cast<float4*>(out)[i] = y;
    }
}

// BatchNorm backward, the input gradient: dx = gamma rstd (dy - dbeta / M - xhat dgamma / M), M the tape's valid rows; dx == dy is
// allowed.  The rows of padded frames are written as zeros.
__global__ __launch_bounds__(256) void xfmr_bn_bwd_dx_kernel(const float* __restrict__ x, const float* dy, const float* __restrict__ stats,
                                                             const float* __restrict__ gamma, const float* __restrict__ dgamma,
                                                             const float* __restrict__ dbeta, float* dx, long long n, int F, const BigruTapeHeader* hdr,
                                                             const int* __restrict__ tape_lens, int T, const XfmrLayout lay) {
    const float inv_m = 1.f / (float)hdr->M;
    const int* const lens = bigru_tape_lens(hdr, tape_lens);
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        if (!xfmr_elem_valid(lay, lens, e, F, T)) {
            dx[e] = 0.f;
            continue;
        }
        const int c = (int)(e % F);
        const float rstd = stats[2 * F + c];
        const float xhat = (x[e] - stats[c]) * rstd;
        dx[e] = gamma[c] * rstd * (dy[e] - dbeta[c] * inv_m - xhat * dgamma[c] * inv_m);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Elementwise pieces over rows (n % 4 == 0; element index = the row-major index in (B, T, C)).  site < 0: no dropout.
//   xfmr_add_drop_kernel   out = x + t factor(site, e)                 the residual joins of an encoder layer (dropout1, dropout2)
//   xfmr_gate_kernel       out = a > 0 ? d factor(site, e) : 0         ReLU' (a: the ReLU's output) and the dropout behind it; a = null: dropout only
// Rows are `width` floats (width % 4 == 0); on a ragged tape the rows of padded frames are written as zeros and their inputs not read.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void xfmr_add_drop_kernel(const float* __restrict__ x, const float* __restrict__ t, float* __restrict__ out, long long n,
                                                            const BigruTapeHeader* hdr, int site, const int* __restrict__ tape_lens, int width, int T,
                                                            const XfmrLayout lay) {
    const XfmrDrop drop(hdr, site);
    const int* const lens = bigru_tape_lens(hdr, tape_lens);
    for (long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; e < n; e += (long long)gridDim.x * 1024) {
        if (!xfmr_elem_valid(lay, lens, e, width, T)) {
            *reinterpret_cast<float4*>(out + e) = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        const unsigned long long de = xfmr_drop_elem(lay, e, width);
        const float4 a = *reinterpret_cast<const float4*>(x + e), v = *reinterpret_cast<const float4*>(t + e);
        *reinterpret_cast<float4*>(out + e) = make_float4(a.x + v.x * drop(de), a.y + v.y * drop(de + 1), a.z + v.z * drop(de + 2), a.w + v.w * drop(de + 3));
    }
}

__global__ __launch_bounds__(256) void xfmr_gate_kernel(const float* a, const float* d, float* out, long long n, const BigruTapeHeader* hdr, int site,
                                                        const int* __restrict__ tape_lens, int width, int T, const XfmrLayout lay) {
    const XfmrDrop drop(hdr, site < 0 ? 0 : site);
    const int* const lens = bigru_tape_lens(hdr, tape_lens);
    for (long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; e < n; e += (long long)gridDim.x * 1024) {
        if (!xfmr_elem_valid(lay, lens, e, width, T)) {
            *reinterpret_cast<float4*>(out + e) = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        float4 v = *reinterpret_cast<const float4*>(d + e);
        if (site >= 0) {
            const unsigned long long de = xfmr_drop_elem(lay, e, width);
            v.x *= drop(de);
            v.y *= drop(de + 1);
            v.z *= drop(de + 2);
            v.w *= drop(de + 3);
        }
        if (a) {
            const float4 m = *reinterpret_cast<const float4*>(a + e);
            v = make_float4(m.x > 0.f ? v.x : 0.f, m.y > 0.f ? v.y : 0.f, m.z > 0.f ? v.z : 0.f, m.w > 0.f ? v.w : 0.f);
        }
        *reinterpret_cast<float4*>(out + e) = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// LayerNorm backward: one wave per row, mean and rstd recomputed from the saved pre-norm row exactly as xfmr_ln_kernel computes them (and
// left in rowstats for the column sums of d gamma / d beta): with g = dy gamma and xhat = (x - mean) rstd,
//     dx = rstd (g - mean(g) - xhat mean(g xhat)).     F <= 1024, a multiple of 4.  dx == dy is allowed.
// A padded frame's row (ragged tape): dx is written as zeros, nothing is read, and its rowstats stay unwritten (the column sums skip it).
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void xfmr_ln_bwd_kernel(const float* __restrict__ x, const float* dy, const float* __restrict__ gamma, float* dx,
                                                          float* __restrict__ rowstats, long long M, int F, const BigruTapeHeader* hdr,
                                                          const int* __restrict__ tape_lens, int T, const XfmrLayout lay) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int nv = F >> 2;
    if (!xfmr_row_valid(lay, bigru_tape_lens(hdr, tape_lens), row, T)) {
        for (int i = lane; i < nv; i += 64) reinterpret_cast<float4*>(dx + row * F)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const float4* xr = reinterpret_cast<const float4*>(x + row * F);
    const float4* dr = reinterpret_cast<const float4*>(dy + row * F);
    const float4* gm = reinterpret_cast<const float4*>(gamma);
    float4 v[4], gv[4];
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = lane + 64 * j;
        v[j] = i < nv ? xr[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        sum += (v[j].x + v[j].y) + (v[j].z + v[j].w);
    }
    const float mean = xfmr_wave_sum(sum) / (float)F;
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (lane + 64 * j >= nv) continue;
        const float a = v[j].x - mean, bb = v[j].y - mean, cc = v[j].z - mean, d = v[j].w - mean;
        sq += (a * a + bb * bb) + (cc * cc + d * d);
    }
    const float rstd = 1.f / sqrtf(xfmr_wave_sum(sq) / (float)F + 1e-5f);
    float sg = 0.f, sgx = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = lane + 64 * j;
        gv[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i >= nv) continue;
        const float4 d = dr[i], w = gm[i];
        gv[j] = make_float4(d.x * w.x, d.y * w.y, d.z * w.z, d.w * w.w);
        v[j] = make_float4((v[j].x - mean) * rstd, (v[j].y - mean) * rstd, (v[j].z - mean) * rstd, (v[j].w - mean) * rstd);
        sg += (gv[j].x + gv[j].y) + (gv[j].z + gv[j].w);
        sgx += (gv[j].x * v[j].x + gv[j].y * v[j].y) + (gv[j].z * v[j].z + gv[j].w * v[j].w);
    }
    const float mg = xfmr_wave_sum(sg) / (float)F, mgx = xfmr_wave_sum(sgx) / (float)F;
    float4* out = reinterpret_cast<float4*>(dx + row * F);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = lane + 64 * j;
        if (i >= nv) continue;
        out[i] = make_float4(rstd * (gv[j].x - mg - v[j].x * mgx), rstd * (gv[j].y - mg - v[j].y * mgx), rstd * (gv[j].z - mg - v[j].z * mgx),
                             rstd * (gv[j].w - mg - v[j].w * mgx));
    }
    if (lane == 0) {
        rowstats[2 * row] = mean;
        rowstats[2 * row + 1] = rstd;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Between the reference's layouts and the fused GEMMs'.
// ---------------------------------------------------------------------------------------------------------------------------
// xfmr_rows_kernel by the tape's frame counts: dout (B, C, T) -> rows [b T + t][Cp]
__global__ __launch_bounds__(256) void xfmr_drows_kernel(const float* __restrict__ x, float* __restrict__ rows, const BigruTapeHeader* hdr,
                                                         const int* __restrict__ tape_lens, int C, int Cp, int T, const XfmrLayout lay) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z, c0 = blockIdx.y * 32, t0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int len = bigru_len(bigru_tape_lens(hdr, tape_lens), b, T);
    for (int r = ty; r < 32; r += 8) {
        const int c = c0 + r, t = t0 + tx;
        tile[r][tx] = (c < C && t < len) ? x[((size_t)b * C + c) * T + t] : 0.f;
    }
    __syncthreads();
    const size_t base = xfmr_seq_row0(lay, b, T);
    const int tw = lay.row0 ? len : T;  // (packed: a sequence's own rows; the gap rows are xfmr_zero_gaps_kernel's)
    for (int r = ty; r < 32; r += 8) {
        const int t = t0 + r, c = c0 + tx;
        if (t < tw && c < Cp) rows[(base + t) * Cp + c] = tile[tx][r];
    }
}

// rows [b T + t][Cp] -> dx (B, C, T): the input gradient in the reference's layout; a padded frame's (ragged tape) is zero and its row,
// which holds what the k = 3 data gradient spilled over the sequence's end, is not read
__global__ __launch_bounds__(256) void xfmr_unrows_kernel(const float* __restrict__ rows, float* __restrict__ dx, const BigruTapeHeader* hdr,
                                                          const int* __restrict__ tape_lens, int C, int Cp, int T, const XfmrLayout lay) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z, c0 = blockIdx.y * 32, t0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int len = bigru_len(bigru_tape_lens(hdr, tape_lens), b, T);
    const size_t base = xfmr_seq_row0(lay, b, T);
    for (int r = ty; r < 32; r += 8) {
        const int t = t0 + r, c = c0 + tx;
        tile[r][tx] = (t < len && c < Cp) ? rows[(base + t) * Cp + c] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int c = c0 + r, t = t0 + tx;
        if (c < C && t < T) dx[((size_t)b * C + c) * T + t] = tile[tx][r];
    }
}

// w_q | w_k | w_v, each (8, F, d), -> the q | k | v GEMM's (3 F, F) weight: row (s 8 + h) d + a, column f is w_s[h, f, a]; back == 1: the
// weight gradient the other way
__global__ __launch_bounds__(256) void xfmr_qkv_weight_kernel(float* __restrict__ wq, float* __restrict__ wk, float* __restrict__ wv,
                                                              float* __restrict__ fused, int F, int d, int back) {
    const long long n = (long long)3 * F * F;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int row = (int)(i / F), f = (int)(i - (long long)row * F);
        const int s = row / F, ha = row - s * F, hh = ha / d, a = ha - hh * d;
        float* const w = s == 0 ? wq : s == 1 ? wk : wv;
        const size_t e = ((size_t)hh * F + f) * d + a;
        if (back) w[e] = fused[i];
        else fused[i] = w[e];
    }
}

// Conv1d + eval-mode BatchNorm1d folded as hificar_xfmr_finalize folds them on the host (same double arithmetic): wf (cout, cols), bf (cout)
__global__ __launch_bounds__(256) void xfmr_fold_kernel(const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, const float* __restrict__ mean, const float* __restrict__ var,
                                                        float* __restrict__ wf, float* __restrict__ bf, int cols) {
    const int o = blockIdx.x;
    const double s = (double)gamma[o] / sqrt((double)var[o] + 1e-5);
    for (int k = threadIdx.x; k < cols; k += 256) wf[(size_t)o * cols + k] = (float)((double)w[(size_t)o * cols + k] * s);
    if (threadIdx.x == 0) bf[o] = (float)(((double)b[o] - (double)mean[o]) * s + (double)beta[o]);
}

}  // namespace hificar

#include "hificar_xfmr_pack16.hip.h"  // the bf16x3 training arithmetic's two passes
