// The building blocks the bf16 attention kernels share (xfmr_attn16_kernel, xfmr_attn16_train_kernel, xfmr_attn16_bwd_q_kernel,
// xfmr_attn16_bwd_k_kernel, xfmr_demb16_partial_kernel; hubert_attn16_kernel, without the band).  Their common plan: a query (or a key) is a lane column, blocks are 64 rows, the
// next block is in flight global -> registers while the current one is multiplied, every product is hi.hi + hi.lo + lo.hi on
// v_mfma_f32_16x16x32_bf16 with fp32 accumulation, hi = bf16(x), lo = bf16(x - hi).
//
// The row image.  [64][hi: DP bf16 | lo: DP bf16 | 32 bytes], DP = D rounded up to 32; the padded channels are zeros (written once, never
// staged over).  ONE image serves both kinds of read:
//   row operand         lane (c, g) reads channels 32 ks + 8 g .. + 7 of row 16 sb + c with one ds_read_b128 per half; the pitch PK = 4 DP + 32
//                       is 2 (mod 8) 16-byte slots, so the 16 lanes of every ds_read_b128 lane group ({0-3, 12-15, 20-27}, ...: rows c with
//                       chunk g) fall in 16 different slots of the 256-byte bank row (with a 16-byte pad each group is 2-way)
//   transposed operand  ds_read_b64_tr_b16 of 4 rows x 16 channels per 16 lanes, 32 rows per MFMA: the B operand's slots 8 g + 0 .. 3 are the
//                       first 16-row accumulator's registers (rows 4 g + i) and 8 g + 4 .. 7 the second's (rows 16 + 4 g + i), split and
//                       packed in registers — P, dS and Pd never go through LDS on their way to a product.  PK is 32 or 160 (mod 256), so
//                       the 8 rows x 32 bytes a 32-lane half reads start at 8 different multiples of 32 in the bank row
// so both are conflict-free by the bank rule at every head size.  Every transposed read is 8-byte aligned and needs EXEC all ones: no
// lane leaves before the end, the only branches around one are wave-uniform (a scalar condition), and no helper below returns early.
// Arrays handed to a helper (s[4], o[NM], qh[NK]) are indexed by unrolled compile-time indices only: they stay in registers.
#pragma once
#include "hificar_xfmr_kernels.hip.h"

namespace hificar {

constexpr int kXfmrTabPad = 208;  // rows of one head's split table: 13 tiles of 16, rows 199 .. 207 zeros

// a layer's split position tables, [8][208][d] bf16 each
struct XfmrTab16 {
    const uint16_t* hi;
    const uint16_t* lo;
};

template <int D>
struct XfmrAttn16Row {
    static constexpr int DP = (D + 31) / 32 * 32;  // channels of an LDS row
    static constexpr int PK = 4 * DP + 32;         // bytes per row (hi | lo | pad)
    static constexpr int NK = DP / 32, NM = D / 16;  // k-steps of a row-operand product, 16-channel tiles of a transposed one
    static constexpr int img_bytes = kXfmrKB * PK;
};

struct XfmrSplit {
    __bf16 hi, lo;
};
__device__ __forceinline__ XfmrSplit xfmr_split(float x) {
    const __bf16 hi = (__bf16)x;
    return {hi, (__bf16)(x - (float)hi)};
}
template <int N, class V>
__device__ __forceinline__ void xfmr_split_n(const float (&x)[N], V& hi, V& lo) {
#pragma unroll
    for (int e = 0; e < N; ++e) {
        const XfmrSplit s = xfmr_split(x[e]);
        hi[e] = s.hi;
        lo[e] = s.lo;
    }
}
// eight channels of an fp32 row as a split 16-byte piece
__device__ __forceinline__ void xfmr_split8(const float4& a, const float4& b, bf16x8& hi, bf16x8& lo) {
    const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    xfmr_split_n(x, hi, lo);
}
// two 16-row accumulators as the split B operand of a 32-row step
__device__ __forceinline__ void xfmr_split_b(const f32x4& x0, const f32x4& x1, bf16x8& hi, bf16x8& lo) {
    const float x[8] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
    xfmr_split_n(x, hi, lo);
}

__device__ __forceinline__ void xfmr_attn16_zero(char* lds, int bytes, int tid) {
    for (int i = tid; i < bytes / 16; i += 256) *reinterpret_cast<uint4*>(lds + 16 * i) = make_uint4(0u, 0u, 0u, 0u);
}

// this lane's address in an image of pitch P as a row operand: row c of a 16-row step, its 8 channels of k-step 0
template <int P>
__device__ __forceinline__ const char* xfmr_attn16_row_ptr(const char* img, int c, int g) { return img + c * P + 16 * g; }
// ... and for the transposed read of rows 4 g .. 4 g + 3, channels 0 .. 15: row 4 g + (c >> 2), channels 4 (c & 3) ..
template <int P>
__device__ __forceinline__ const char* xfmr_attn16_tr_ptr(const char* img, int c, int g) { return img + (4 * g + (c >> 2)) * P + 8 * (c & 3); }

// (wave-uniform) step t of a block of n rows, rows x32 .. x32 + 31, meets the band of the wave's columns w0 .. w0 + 15
__device__ __forceinline__ bool xfmr_attn16_step_meets(int t, int n, int x32, int w0) {
    return 32 * t < n && x32 + 31 >= w0 - (kXfmrRel - 1) && x32 <= w0 + 15 + (kXfmrRel - 1);
}
// (per element) the lane's column exists, the row is inside the block's count, and their relative position has a table row
__device__ __forceinline__ bool xfmr_attn16_in_band(bool col_ok, int row, int row_end, int rel) {
    return col_ok && row < row_end && rel >= 0 && rel < kXfmrTab;
}

typedef short xfmr_s16x4 __attribute__((ext_vector_type(4)));

// 16 channels x (rows 4 g .. 4 g + 3 and 16 + 4 g .. + 3) of an image of pitch P as the A operand; `a`: this lane's address of the first block
template <int P>
__device__ __forceinline__ bf16x8 xfmr_attn16_vfrag(const char* a) {
    typedef __attribute__((address_space(3))) xfmr_s16x4* lds_ptr;
    const xfmr_s16x4 x0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(a));
    const xfmr_s16x4 x1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(a + 16 * P));
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(x0, x1, 0, 1, 2, 3, 4, 5, 6, 7));
}

// acc += A B with both operands split: the two cross terms, then hi . hi
__device__ __forceinline__ f32x4 xfmr_attn16_mfma3(bf16x8 ah, bf16x8 al, bf16x8 bh, bf16x8 bl, f32x4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, acc, 0, 0, 0);
}

// acc += A_rows . b over the row image's k-steps; `a`: this lane's address of the 16-row step (xfmr_attn16_row_ptr)
template <int D>
__device__ __forceinline__ f32x4 xfmr_attn16_rows_dot(const char* a, const bf16x8* bh, const bf16x8* bl, f32x4 acc) {
    using R = XfmrAttn16Row<D>;
#pragma unroll
    for (int ks = 0; ks < R::NK; ++ks)
        acc = xfmr_attn16_mfma3(*reinterpret_cast<const bf16x8*>(a + 64 * ks), *reinterpret_cast<const bf16x8*>(a + 2 * R::DP + 64 * ks), bh[ks], bl[ks], acc);
    return acc;
}

// o[j] += A^T_tile(j) . b over NM 16-channel tiles of an image with row pitch P whose lo half starts LO bytes behind the hi half; `a`: this
// lane's address of the 32-row step (xfmr_attn16_tr_ptr)
template <int NM, int P, int LO>
__device__ __forceinline__ void xfmr_attn16_tr_dot(const char* a, bf16x8 bh, bf16x8 bl, f32x4* o) {
#pragma unroll
    for (int j = 0; j < NM; ++j) o[j] = xfmr_attn16_mfma3(xfmr_attn16_vfrag<P>(a + 32 * j), xfmr_attn16_vfrag<P>(a + LO + 32 * j), bh, bl, o[j]);
}

// this lane's B operand of a product over channels: x[32 ks + 8 g .. + 7] of an fp32 row, split (zeros: !ok, padded channels)
template <int D>
__device__ __forceinline__ void xfmr_attn16_row_operand(const float* row, bool ok, int g, bf16x8* hi, bf16x8* lo) {
#pragma unroll
    for (int ks = 0; ks < XfmrAttn16Row<D>::NK; ++ks) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        if (ok && 32 * ks + 8 * g < D) {
            a = *reinterpret_cast<const float4*>(row + 32 * ks + 8 * g);
            b = *reinterpret_cast<const float4*>(row + 32 * ks + 8 * g + 4);
        }
        xfmr_split8(a, b, hi[ks], lo[ks]);
    }
}

// table rows r0 .. r0 + 63 of head h -> a row image (rows at or past 208: zeros).  Between two barriers of the caller's.
template <int D>
__device__ __forceinline__ void xfmr_attn16_stage_tab(char* kimg, const XfmrTab16 tab, int h, int r0, int tid) {
    using R = XfmrAttn16Row<D>;
    constexpr int CPR = D / 8;
    for (int u = tid; u < kXfmrKB * 2 * CPR; u += 256) {
        const int r = u / (2 * CPR), w = u - r * (2 * CPR), half = w / CPR, ch = w - half * CPR;
        uint4 x = make_uint4(0u, 0u, 0u, 0u);
        if (r0 + r < kXfmrTabPad) x = *reinterpret_cast<const uint4*>((half ? tab.lo : tab.hi) + ((size_t)h * kXfmrTabPad + r0 + r) * D + 8 * ch);
        *reinterpret_cast<uint4*>(kimg + r * R::PK + half * 2 * R::DP + 16 * ch) = x;
    }
}

// positional logits of the wave's 16 queries: mypos[r] = Q[q] . E[r], the table staged through the K image (every thread of the workgroup)
template <int D>
__device__ __forceinline__ void xfmr_attn16_pos(char* kimg, float* mypos, const char* arow, const XfmrTab16 tab, int h, const bf16x8* qh, const bf16x8* ql,
                                                int tid, int g) {
    for (int r0 = 0; r0 < kXfmrTabPad; r0 += kXfmrKB) {
        __syncthreads();
        xfmr_attn16_stage_tab<D>(kimg, tab, h, r0, tid);
        __syncthreads();
#pragma unroll
        for (int sb = 0; sb < 4; ++sb) {
            if (r0 + 16 * sb >= kXfmrTabPad) continue;
            const f32x4 acc = xfmr_attn16_rows_dot<D>(arow + 16 * sb * XfmrAttn16Row<D>::PK, qh, ql, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = r0 + 16 * sb + 4 * g + i;
                if (r < kXfmrTab) mypos[r] = acc[i];
            }
        }
    }
}

// One 64-key block of the forward: S^T = K Q^T in four 16-key tiles (key kb + 16 sb + 4 g + i in s[sb][i]), scale and positional logit,
// the online softmax's update of this lane's query (m: running maximum, -inf before the first key; l: denominator).  Leaves the
// exponentials in s (zeros where `valid` has no bit) and returns alpha, the factor the caller's accumulators of earlier blocks take.
//   valid  bit 4 sb + i: the key is in this query's band and inside the sequence
//   act    (wave-uniform) the 32-key step meets the band of the wave's queries qw .. qw + 15
// BAND = false (hubert_attn16_kernel: full attention, no position table): every key of the block's n counts, a step is active while it holds
// one of them, and the logit is the scaled product alone; mypos, q and qw are not read.
template <int D, bool BAND = true>
__device__ __forceinline__ float xfmr_attn16_scores(const char* arow, const bf16x8* qh, const bf16x8* ql, const float* mypos, float scale, int kb, int n,
                                                    int q, int qw, bool qok, int g, f32x4 (&s)[4], unsigned& valid, bool (&act)[2], float& m, float& l) {
    valid = 0;
    float mb = -INFINITY;
#pragma unroll
    for (int t = 0; t < 2; ++t) act[t] = BAND ? xfmr_attn16_step_meets(t, n, kb + 32 * t, qw) : 32 * t < n;
#pragma unroll
    for (int sb = 0; sb < 4; ++sb) {
        s[sb] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (!act[sb >> 1]) continue;
        s[sb] = xfmr_attn16_rows_dot<D>(arow + 16 * sb * XfmrAttn16Row<D>::PK, qh, ql, s[sb]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = kb + 16 * sb + 4 * g + i;
            const int rel = k - q + (kXfmrRel - 1);
            if (BAND ? xfmr_attn16_in_band(qok, k, kb + n, rel) : qok && k < kb + n) {
                const float v = BAND ? s[sb][i] * scale + mypos[rel] : s[sb][i] * scale;
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
    return alpha;
}

// This thread's share of a 64-row block of two fp32 tensors, fetched to registers and split when it is committed to two row images:
// D / 16 pieces of 8 channels.  Piece u = tid + 256 i is piece (u mod 2 CPR) of row u / (2 CPR); a row's pieces are the first tensor's,
// then the second's, CPR = D / 8 each.  Source and destination offsets are the same for every block.  Src::offset(second, r, F): where row
// r of a block starts in its tensor.
struct XfmrAttn16SrcKV {  // K | V of q | k | v rows: one tensor
    static __device__ __forceinline__ int offset(int second, int r, int F) { return r * 3 * F + (second + 1) * F; }
};
struct XfmrAttn16SrcDoQ {  // dO rows, then Q of q | k | v rows
    static __device__ __forceinline__ int offset(int second, int r, int F) { return r * (second ? 3 * F : F); }
};
template <int D, class Src>
struct XfmrAttn16Stage {
    using R = XfmrAttn16Row<D>;
    static constexpr int NP = D / 16, CPR = D / 8;
    int row[NP], src[NP], dst[NP];
    bool second[NP];
    float4 a[NP], b[NP];
    __device__ __forceinline__ void init(int tid, int F, int h) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int u = tid + 256 * i, r = u / (2 * CPR), w = u - r * (2 * CPR), part = w / CPR, ch = w - part * CPR;
            row[i] = r;
            second[i] = part != 0;
            src[i] = Src::offset(part, r, F) + h * D + 8 * ch;
            dst[i] = part * R::img_bytes + r * R::PK + 16 * ch;
        }
    }
    // rows at or past n are zeros, never read: the rows past a sequence's length hold whatever was there
    __device__ __forceinline__ void fetch(const float* t0, const float* t1, int n) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            a[i] = b[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row[i] < n) {
                const float* s = (second[i] ? t1 : t0) + src[i];
                a[i] = *reinterpret_cast<const float4*>(s);
                b[i] = *reinterpret_cast<const float4*>(s + 4);
            }
        }
    }
    __device__ __forceinline__ void fetch(const float* t, int n) { fetch(t, t, n); }
    __device__ __forceinline__ void commit(char* lds) const {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            bf16x8 hi, lo;
            xfmr_split8(a[i], b[i], hi, lo);
            *reinterpret_cast<bf16x8*>(lds + dst[i]) = hi;
            *reinterpret_cast<bf16x8*>(lds + dst[i] + 2 * R::DP) = lo;
        }
    }
};

}  // namespace hificar
