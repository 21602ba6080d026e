// The query-tiled attention kernels of the bf16x3wa training arithmetic (hificar_xfmr_set_train_precision, HIFICAR_PREC_BF16X3WA): the
// training forward (xfmr_attn16_train_kernel: profile row xfmr_attn16_kernel<train>) and the query-tiled backward (xfmr_attn16_bwd_q_kernel)
// with xfmr_attn16_kernel's plan — a query is a lane column, 64-key blocks, the next block in flight global -> registers while the current one
// is multiplied, every banded product as hi.hi + hi.lo + lo.hi on v_mfma_f32_16x16x32_bf16 with fp32 accumulation, P and dS never through LDS
// on their way to the V / K products.  The key-tiled kernels (xfmr_attn_bwd_k_kernel, xfmr_demb_partial_kernel) stay exact fp32 and read the
// banded fp32 dS / Pd buffers this backward writes exactly as xfmr_attn_bwd_q_kernel lays them out.
//
// Operands.  The tape keeps fp32 q | k | v rows: a fetched block travels as fp32 in registers and is split when it is committed to LDS
// (hi = bf16(x), lo = bf16(x - hi)).  Q and dO of the lane's own query are split once, in registers.  The position tables arrive split and
// padded ([8][208][d] hi and lo, rows 199 .. 207 zeros: xfmr_split_tab_kernel, behind every parameter hand-over).
//
// LDS image (bytes): K rows [64][hi: DP bf16 | lo: DP bf16 | 32], V rows the same, pos[64][211] fp32; DP = D rounded up to 32, the padded
// channels are zeros (written once, never staged over).  ONE image per tensor serves both kinds of read:
//   row operand (S^T = K Q^T, E Q^T, dPd^T = V dO^T)   one ds_read_b128 per half; the pitch PK = 4 DP + 32 is 2 (mod 8) 16-byte slots, the 16
//                                                      lanes of a lane group fall in 16 different slots of the 256-byte bank row
//   transposed operand (O^T += V^T Pd^T, dQ^T += K^T dS^T, dQ^T += E^T dS^T)   ds_read_b64_tr_b16 of 4 rows x 16 channels per 16 lanes; PK is
//                                                      32 or 160 (mod 256), so the 8 rows x 32 bytes a 32-lane half reads start at 8 different
//                                                      multiples of 32 in the bank row (r 32 or r 160 mod 256, r = 0 .. 7: all distinct)
// so both are conflict-free by the bank rule at every head size, and the largest image (D = 128) is 2 x 34 816 + 54 016 = 123 648 bytes.
// The transposed read needs EXEC all ones: no lane leaves before the end, and the only branches around it are wave-uniform.
// The order of every sum depends on the query's position and the sequence's length only.
#pragma once
#include "hificar_xfmr_attn16.hip.h"
#include "hificar_xfmr_train_kernels.hip.h"

namespace hificar {

// emb [8][199][d] fp32 -> hi, lo [8][208][d] bf16 (rows 199 .. 207: zero bits)
__global__ __launch_bounds__(256) void xfmr_split_tab_kernel(const float* __restrict__ emb, uint16_t* __restrict__ hi, uint16_t* __restrict__ lo, int d) {
    const int n = kXfmrHeads * kXfmrTabPad * d;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int ch = i % d, hr = i / d, r = hr % kXfmrTabPad, h = hr / kXfmrTabPad;
        const float x = r < kXfmrTab ? emb[((size_t)h * kXfmrTab + r) * d + ch] : 0.f;
        const __bf16 a = (__bf16)x, b = (__bf16)(x - (float)a);
        hi[i] = __builtin_bit_cast(uint16_t, a);
        lo[i] = __builtin_bit_cast(uint16_t, b);
    }
}

struct XfmrAttn16TrainParams {
    XfmrAttnParams f;        // the fp32 kernel's (emb unused)
    const uint16_t* emb_hi;  // [8][208][d] bf16
    const uint16_t* emb_lo;
};

struct XfmrAttn16BwdParams {
    XfmrAttnBwdParams b;     // the fp32 kernel's (emb unused)
    const uint16_t* emb_hi;
    const uint16_t* emb_lo;
};

template <int D>
struct XfmrAttn16TrainLds {
    static constexpr int DP = (D + 31) / 32 * 32;  // channels of an LDS row
    static constexpr int PK = 4 * DP + 32;         // bytes per row (hi | lo | pad)
    static constexpr int img_bytes = kXfmrKB * PK;
    static constexpr size_t bytes = (size_t)2 * img_bytes + (size_t)kXfmrTQ * kXfmrPosPitch * sizeof(float);
};

__device__ __forceinline__ void xfmr_split8(const float4& a, const float4& b, bf16x8& hi, bf16x8& lo) {
    const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        hi[e] = (__bf16)x[e];
        lo[e] = (__bf16)(x[e] - (float)hi[e]);
    }
}

// This thread's share of a 64-key block: D / 16 pieces of 8 channels.  Piece u = tid + 256 i is piece (u mod 2 CPR) of key row u / (2 CPR); a
// row's pieces are K, then V, CPR = D / 8 each.  Source and destination offsets are the same for every block.
template <int D>
struct XfmrAttn16Stage {
    using L = XfmrAttn16TrainLds<D>;
    static constexpr int NP = D / 16, CPR = D / 8;
    int row[NP], src[NP], dst[NP];
    float4 a[NP], b[NP];
    __device__ __forceinline__ void init(int tid, int F, int h) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int u = tid + 256 * i, r = u / (2 * CPR), w = u - r * (2 * CPR), part = w / CPR, ch = w - part * CPR;
            row[i] = r;
            src[i] = r * 3 * F + (part + 1) * F + h * D + 8 * ch;
            dst[i] = part * L::img_bytes + r * L::PK + 16 * ch;
        }
    }
    // rows at or past n are zeros, never read: the rows past a sequence's length hold whatever was there
    __device__ __forceinline__ void fetch(const float* base, int n) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            a[i] = b[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row[i] < n) {
                a[i] = *reinterpret_cast<const float4*>(base + src[i]);
                b[i] = *reinterpret_cast<const float4*>(base + src[i] + 4);
            }
        }
    }
    __device__ __forceinline__ void commit(char* lds) const {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            bf16x8 hi, lo;
            xfmr_split8(a[i], b[i], hi, lo);
            *reinterpret_cast<bf16x8*>(lds + dst[i]) = hi;
            *reinterpret_cast<bf16x8*>(lds + dst[i] + 2 * L::DP) = lo;
        }
    }
};

// this lane's B operand of a product over channels: x[32 ks + 8 g .. + 7] of an fp32 row, split (zeros: !ok, padded channels)
template <int D>
__device__ __forceinline__ void xfmr_attn16_row_operand(const float* row, bool ok, int g, bf16x8* hi, bf16x8* lo) {
#pragma unroll
    for (int ks = 0; ks < (D + 31) / 32; ++ks) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        if (ok && 32 * ks + 8 * g < D) {
            a = *reinterpret_cast<const float4*>(row + 32 * ks + 8 * g);
            b = *reinterpret_cast<const float4*>(row + 32 * ks + 8 * g + 4);
        }
        xfmr_split8(a, b, hi[ks], lo[ks]);
    }
}

// table rows r0 .. r0 + 63 of head h -> the K image (rows at or past 208: zeros).  Between two barriers of the caller's.
template <int D>
__device__ __forceinline__ void xfmr_attn16_stage_tab(char* kimg, const uint16_t* emb_hi, const uint16_t* emb_lo, int h, int r0, int tid) {
    using L = XfmrAttn16TrainLds<D>;
    constexpr int CPR = D / 8;
    for (int u = tid; u < kXfmrKB * 2 * CPR; u += 256) {
        const int r = u / (2 * CPR), w = u - r * (2 * CPR), half = w / CPR, ch = w - half * CPR;
        uint4 x = make_uint4(0u, 0u, 0u, 0u);
        if (r0 + r < kXfmrTabPad) x = *reinterpret_cast<const uint4*>((half ? emb_lo : emb_hi) + ((size_t)h * kXfmrTabPad + r0 + r) * D + 8 * ch);
        *reinterpret_cast<uint4*>(kimg + r * L::PK + half * 2 * L::DP + 16 * ch) = x;
    }
}

// positional logits of the wave's 16 queries: mypos[r] = Q[q] . E[r], the table staged through the K image (every thread of the workgroup)
template <int D>
__device__ __forceinline__ void xfmr_attn16_pos(char* kimg, float* mypos, const char* arow, const uint16_t* emb_hi, const uint16_t* emb_lo, int h,
                                                const bf16x8* qh, const bf16x8* ql, int tid, int g) {
    using L = XfmrAttn16TrainLds<D>;
    constexpr int NK = L::DP / 32;
    for (int r0 = 0; r0 < kXfmrTabPad; r0 += kXfmrKB) {
        __syncthreads();
        xfmr_attn16_stage_tab<D>(kimg, emb_hi, emb_lo, h, r0, tid);
        __syncthreads();
#pragma unroll
        for (int sb = 0; sb < 4; ++sb) {
            if (r0 + 16 * sb >= kXfmrTabPad) continue;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const char* a = arow + 16 * sb * L::PK;
#pragma unroll
            for (int ks = 0; ks < NK; ++ks)
                acc = xfmr_attn16_mfma3(*reinterpret_cast<const bf16x8*>(a + 64 * ks), *reinterpret_cast<const bf16x8*>(a + 2 * L::DP + 64 * ks), qh[ks], ql[ks], acc);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = r0 + 16 * sb + 4 * g + i;
                if (r < kXfmrTab) mypos[r] = acc[i];
            }
        }
    }
}

// eight fp32 values as a split B operand
__device__ __forceinline__ void xfmr_split_b(const f32x4& x0, const f32x4& x1, bf16x8& hi, bf16x8& lo) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float x = e < 4 ? x0[e & 3] : x1[e & 3];
        hi[e] = (__bf16)x;
        lo[e] = (__bf16)(x - (float)hi[e]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The training forward: xfmr_attn_kernel<D, true>'s statements (dropout factor on the kept probabilities before P V with XfmrDrop's element
// index, L = m + log l per query, zeros on the `out` rows of padded frames, the packed layout) on xfmr_attn16_kernel's products.
// ---------------------------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void xfmr_attn16_train_kernel(const XfmrAttn16TrainParams pp) {
    extern __shared__ __attribute__((aligned(16))) char xfmr16_lds[];
    using L = XfmrAttn16TrainLds<D>;
    constexpr int DP = L::DP, PK = L::PK, NK = DP / 32, NM = D / 16, PP = kXfmrPosPitch;
    static_assert(kXfmrKB == 64 && kXfmrTQ == 64, "the staging shares are for 64-key blocks and 256 threads");
    const XfmrAttnParams& p = pp.f;
    char* const kimg = xfmr16_lds;
    char* const vimg = xfmr16_lds + L::img_bytes;
    float* const pos = reinterpret_cast<float*>(xfmr16_lds + 2 * L::img_bytes);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, g = lane >> 4;
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * kXfmrTQ;
    const int len = p.lengths ? min(max(p.lengths[b], 0), p.T) : p.T;
    const size_t row0 = xfmr_attn_row0<true>(p, b);
    const size_t F3 = (size_t)3 * p.F;
    const int qw = q0 + wave * 16, q = qw + c;
    const bool qok = q < len;
    if (q0 >= len) {  // (the whole workgroup: no barrier has been reached, nothing staged)
        xfmr_zero_head_row<D>(p.out + (row0 + q) * p.F + h * D + 4 * g, q < p.T && !p.row0);
        return;
    }

    // the padded channels of both images are zeros from here on: the staging never writes them
    for (int i = tid; i < 2 * L::img_bytes / 16; i += 256) *reinterpret_cast<uint4*>(xfmr16_lds + 16 * i) = make_uint4(0u, 0u, 0u, 0u);

    bf16x8 qh[NK], ql[NK];
    xfmr_attn16_row_operand<D>(p.qkv + (row0 + (qok ? q : q0)) * F3 + h * D, qok, g, qh, ql);

    XfmrAttn16Stage<D> st;
    st.init(tid, p.F, h);
    const int k_lo = max(0, q0 - (kXfmrRel - 1));
    const int k_hi = min(len, q0 + kXfmrTQ + (kXfmrRel - 1));
    st.fetch(p.qkv + (row0 + k_lo) * F3, min(kXfmrKB, k_hi - k_lo));  // in flight during the positional product

    float* const mypos = pos + (wave * 16 + c) * PP;
    const char* const arow = kimg + c * PK + 16 * g;  // row c of a 16-row step, this lane's 8 channels of k-step 0
    xfmr_attn16_pos<D>(kimg, mypos, arow, pp.emb_hi, pp.emb_lo, h, qh, ql, tid, g);
    __syncthreads();
    st.commit(xfmr16_lds);
    __syncthreads();

    const XfmrDrop drop(p.hdr, p.site);
    const unsigned long long e0 = ((unsigned long long)(b * kXfmrHeads + h) * p.T + (qok ? q : 0)) * kXfmrTab;
    float m = -INFINITY, l = 0.f;  // running maximum (-inf: no key yet) and denominator of this lane's query
    f32x4 o[NM];
#pragma unroll
    for (int j = 0; j < NM; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // this lane's address in the V image for the transposed read of keys 4 g .. 4 g + 3, channels 0 .. 15: row 4 g + (c >> 2), channels 4 (c & 3) ..
    const char* const vtr = vimg + (4 * g + (c >> 2)) * PK + 8 * (c & 3);

    for (int kb = k_lo; kb < k_hi; kb += kXfmrKB) {
        const int n = min(kXfmrKB, k_hi - kb);
        const bool more = kb + kXfmrKB < k_hi;
        if (more) st.fetch(p.qkv + (row0 + kb + kXfmrKB) * F3, min(kXfmrKB, k_hi - kb - kXfmrKB));  // the next block travels while this one is multiplied

        f32x4 s[4];
        unsigned valid = 0;  // bit 4 sb + i: key kb + 16 sb + 4 g + i is in this query's band and inside the sequence
        bool act[2];         // (wave-uniform) the 32-key step meets the band of the wave's queries qw .. qw + 15
        float mb = -INFINITY;
#pragma unroll
        for (int sb = 0; sb < 4; ++sb) {
            const int k32 = kb + 32 * (sb >> 1);
            if (!(sb & 1)) act[sb >> 1] = 32 * (sb >> 1) < n && k32 + 31 >= qw - (kXfmrRel - 1) && k32 <= qw + 15 + (kXfmrRel - 1);
            s[sb] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (!act[sb >> 1]) continue;
            const char* a = arow + 16 * sb * PK;
#pragma unroll
            for (int ks = 0; ks < NK; ++ks)
                s[sb] = xfmr_attn16_mfma3(*reinterpret_cast<const bf16x8*>(a + 64 * ks), *reinterpret_cast<const bf16x8*>(a + 2 * DP + 64 * ks), qh[ks], ql[ks], s[sb]);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = kb + 16 * sb + 4 * g + i;
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
        // the kept probabilities, scaled, are what V is multiplied with (the denominator sums all of them)
#pragma unroll
        for (int sb = 0; sb < 4; ++sb)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if ((valid >> (4 * sb + i)) & 1u) s[sb][i] *= drop(e0 + (unsigned long long)(kb + 16 * sb + 4 * g + i - q + (kXfmrRel - 1)));
#pragma unroll
        for (int j = 0; j < NM; ++j) o[j] *= alpha;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            if (!act[t]) continue;
            bf16x8 ph, pl;  // slots 0 .. 3: keys 32 t + 4 g + i; slots 4 .. 7: keys 32 t + 16 + 4 g + i
            xfmr_split_b(s[2 * t], s[2 * t + 1], ph, pl);
            const char* a = vtr + 32 * t * PK;
#pragma unroll
            for (int j = 0; j < NM; ++j)
                o[j] = xfmr_attn16_mfma3(xfmr_attn16_vfrag<PK>(a + 32 * j), xfmr_attn16_vfrag<PK>(a + 2 * DP + 32 * j), ph, pl, o[j]);
        }
        if (!more) break;
        __syncthreads();  // every wave has read this block
        st.commit(xfmr16_lds);
        __syncthreads();
    }
    if (!qok) {
        // (w_o's GEMM and its weight gradient read every row of `out`; a padded frame's is zeros)
        xfmr_zero_head_row<D>(p.out + (row0 + q) * p.F + h * D + 4 * g, q < p.T && !p.row0);
        return;
    }
    const float inv = 1.f / l;  // (l >= 1: the query's own key is in its band)
    if (g == 0) p.lse[p.row0 ? (row0 + q) * kXfmrHeads + h : ((size_t)b * kXfmrHeads + h) * p.T + q] = m + logf(l);
    float* orow = p.out + (row0 + q) * p.F + h * D + 4 * g;
#pragma unroll
    for (int j = 0; j < NM; ++j)
        *reinterpret_cast<float4*>(orow + 16 * j) = make_float4(o[j][0] * inv, o[j][1] * inv, o[j][2] * inv, o[j][3] * inv);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The query-tiled backward: xfmr_attn_bwd_q_kernel's statements.  S^T is recomputed with the forward's own sequence of MFMAs (the same
// images, operands and order), so P = exp(S - L) sums to one as the forward's did; dPd^T = V dO^T reads the V image as a row operand;
// dQ^T += K^T dS^T reads the K image transposed, dS split in registers from the accumulators; dQ^T += E^T dS^T sums over the 208 table rows
// in 32-row steps, the table staged through the K image, dS read back as fp32 from the pos rows and split in registers (rows past 198:
// zero operands on both sides).  Delta, the exponential and dS stay fp32; dS and Pd go to the banded fp32 buffers.
// ---------------------------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void xfmr_attn16_bwd_q_kernel(const XfmrAttn16BwdParams pp) {
    extern __shared__ __attribute__((aligned(16))) char xfmr16_lds[];
    using L = XfmrAttn16TrainLds<D>;
    constexpr int DP = L::DP, PK = L::PK, NK = DP / 32, NM = D / 16, PP = kXfmrPosPitch;
    const XfmrAttnBwdParams& p = pp.b;
    char* const kimg = xfmr16_lds;
    char* const vimg = xfmr16_lds + L::img_bytes;
    float* const pos = reinterpret_cast<float*>(xfmr16_lds + 2 * L::img_bytes);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
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

    for (int i = tid; i < 2 * L::img_bytes / 16; i += 256) *reinterpret_cast<uint4*>(xfmr16_lds + 16 * i) = make_uint4(0u, 0u, 0u, 0u);

    bf16x8 qh[NK], ql[NK], doh[NK], dol[NK];
    float delta = 0.f, lq = 0.f;
    {
        const size_t r = row0 + (qok ? q : q0);
        xfmr_attn16_row_operand<D>(p.qkv + r * F3 + h * D, qok, g, qh, ql);
        const float* drow = p.dout + r * p.F + h * D;
        const float* orow = p.o + r * p.F + h * D;
        xfmr_attn16_row_operand<D>(drow, qok, g, doh, dol);
#pragma unroll
        for (int ks = 0; ks < NK; ++ks) {
            if (!(qok && 32 * ks + 8 * g < D)) continue;
#pragma unroll
            for (int e = 0; e < 8; ++e) delta = fmaf(drow[32 * ks + 8 * g + e], orow[32 * ks + 8 * g + e], delta);
        }
        delta += __shfl_xor(delta, 16);
        delta += __shfl_xor(delta, 32);
        if (qok) lq = p.lse[xfmr_band_row(p.lay, row0, b, h, q, p.T)];
    }

    XfmrAttn16Stage<D> st;
    st.init(tid, p.F, h);
    const int k_lo = max(0, q0 - (kXfmrRel - 1));
    const int k_hi = min(len, q0 + kXfmrTQ + (kXfmrRel - 1));
    st.fetch(p.qkv + (row0 + k_lo) * F3, min(kXfmrKB, k_hi - k_lo));

    float* const mypos = pos + (wave * 16 + c) * PP;
    const char* const arow = kimg + c * PK + 16 * g;
    xfmr_attn16_pos<D>(kimg, mypos, arow, pp.emb_hi, pp.emb_lo, h, qh, ql, tid, g);
    __syncthreads();
    st.commit(xfmr16_lds);
    __syncthreads();

    f32x4 o[NM];  // dQ^T of this lane's query: rows 16 j + 4 g + i
#pragma unroll
    for (int j = 0; j < NM; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const char* const vrow = vimg + c * PK + 16 * g;
    const char* const ktr = kimg + (4 * g + (c >> 2)) * PK + 8 * (c & 3);
    const size_t band = xfmr_band_row(p.lay, row0, b, h, qok ? q : q0, p.T) * kXfmrBand;

    for (int kb = k_lo; kb < k_hi; kb += kXfmrKB) {
        const int n = min(kXfmrKB, k_hi - kb);
        const bool more = kb + kXfmrKB < k_hi;
        if (more) st.fetch(p.qkv + (row0 + kb + kXfmrKB) * F3, min(kXfmrKB, k_hi - kb - kXfmrKB));

        f32x4 ds[4];
        bool act[2];
#pragma unroll
        for (int sb = 0; sb < 4; ++sb) {
            const int k32 = kb + 32 * (sb >> 1);
            if (!(sb & 1)) act[sb >> 1] = 32 * (sb >> 1) < n && k32 + 31 >= qw - (kXfmrRel - 1) && k32 <= qw + 15 + (kXfmrRel - 1);
            ds[sb] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (!act[sb >> 1]) continue;
            f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
            const char* ak = arow + 16 * sb * PK;
            const char* av = vrow + 16 * sb * PK;
#pragma unroll
            for (int ks = 0; ks < NK; ++ks)
                s = xfmr_attn16_mfma3(*reinterpret_cast<const bf16x8*>(ak + 64 * ks), *reinterpret_cast<const bf16x8*>(ak + 2 * DP + 64 * ks), qh[ks], ql[ks], s);
#pragma unroll
            for (int ks = 0; ks < NK; ++ks)
                dp = xfmr_attn16_mfma3(*reinterpret_cast<const bf16x8*>(av + 64 * ks), *reinterpret_cast<const bf16x8*>(av + 2 * DP + 64 * ks), doh[ks], dol[ks], dp);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = kb + 16 * sb + 4 * g + i;
                const int rel = k - q + (kXfmrRel - 1);
                const bool ok = qok && k < kb + n && rel >= 0 && rel < kXfmrTab;
                if (ok) {
                    const float pr = expf(s[i] * p.scale + mypos[rel] - lq);
                    const float f = drop((bh * p.T + q) * kXfmrTab + rel);
                    const float dsv = pr * (dp[i] * f - delta);
                    mypos[rel] = dsv;
                    p.pd[band + rel] = pr * f;
                    ds[sb][i] = dsv;
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            if (!act[t]) continue;
            bf16x8 sh, sl;  // slots 0 .. 3: keys 32 t + 4 g + i; slots 4 .. 7: keys 32 t + 16 + 4 g + i
            xfmr_split_b(ds[2 * t], ds[2 * t + 1], sh, sl);
            const char* a = ktr + 32 * t * PK;
#pragma unroll
            for (int j = 0; j < NM; ++j)
                o[j] = xfmr_attn16_mfma3(xfmr_attn16_vfrag<PK>(a + 32 * j), xfmr_attn16_vfrag<PK>(a + 2 * DP + 32 * j), sh, sl, o[j]);
        }
        if (!more) break;
        __syncthreads();  // every wave has read this block
        st.commit(xfmr16_lds);
        __syncthreads();
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

    // dQ^T += E^T dS^T over the table rows, 32 per MFMA (A: E[r][16 j + c] read transposed; B: dS[q = c][r], slots as above)
    for (int r0 = 0; r0 < kXfmrTabPad; r0 += kXfmrKB) {
        __syncthreads();
        xfmr_attn16_stage_tab<D>(kimg, pp.emb_hi, pp.emb_lo, h, r0, tid);
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            if (r0 + 32 * t >= kXfmrTabPad) continue;  // (the whole workgroup)
            f32x4 x0, x1;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int ra = r0 + 32 * t + 4 * g + i, rb = ra + 16;
                x0[i] = ra < kXfmrTab ? mypos[ra] : 0.f;  // (rows 199 ..: the table image holds zeros there, and so does this side)
                x1[i] = rb < kXfmrTab ? mypos[rb] : 0.f;
            }
            bf16x8 sh, sl;
            xfmr_split_b(x0, x1, sh, sl);
            const char* a = ktr + 32 * t * PK;
#pragma unroll
            for (int j = 0; j < NM; ++j)
                o[j] = xfmr_attn16_mfma3(xfmr_attn16_vfrag<PK>(a + 32 * j), xfmr_attn16_vfrag<PK>(a + 2 * DP + 32 * j), sh, sl, o[j]);
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

template <int D>
static hipError_t xfmr_attn16_train_attr() {
    static_assert(XfmrAttn16TrainLds<D>::bytes <= 160 * 1024, "one workgroup per CU");
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&xfmr_attn16_train_kernel<D>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)XfmrAttn16TrainLds<D>::bytes);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&xfmr_attn16_bwd_q_kernel<D>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)XfmrAttn16TrainLds<D>::bytes);
}

template <int D>
static hipError_t xfmr_attn16_train_launch(const XfmrAttn16TrainParams& p, dim3 grid, hipStream_t stream) {
    hipLaunchKernelGGL((xfmr_attn16_train_kernel<D>), grid, dim3(256), XfmrAttn16TrainLds<D>::bytes, stream, p);
    return hipGetLastError();
}

template <int D>
static hipError_t xfmr_attn16_bwd_q_launch(const XfmrAttn16BwdParams& p, dim3 grid, hipStream_t stream) {
    hipLaunchKernelGGL((xfmr_attn16_bwd_q_kernel<D>), grid, dim3(256), XfmrAttn16TrainLds<D>::bytes, stream, p);
    return hipGetLastError();
}

}  // namespace hificar
