// The query-tiled attention kernels of the bf16x3wa training arithmetic (hificar_xfmr_set_train_precision, HIFICAR_PREC_BF16X3WA): the
// training forward (xfmr_attn16_train_kernel: profile row xfmr_attn16_kernel<train>) and the query-tiled backward (xfmr_attn16_bwd_q_kernel)
// with xfmr_attn16_kernel's plan, on the building blocks of hificar_xfmr_attn16_common.hip.h.  The key-tiled kernels (xfmr_attn_bwd_k_kernel,
// xfmr_demb_partial_kernel) stay exact fp32 and read the banded fp32 dS / Pd buffers this backward writes exactly as xfmr_attn_bwd_q_kernel
// lays them out.
//
// Operands.  The tape keeps fp32 q | k | v rows: a fetched block travels as fp32 in registers and is split when it is committed to LDS
// (XfmrAttn16Stage).  Q and dO of the lane's own query are split once, in registers.  The position tables arrive split and padded
// ([8][208][d] hi and lo, rows 199 .. 207 zeros: xfmr_split_tab_kernel, behind every parameter hand-over).
//
// LDS image (bytes): K rows and V rows, one common row image each, then pos[64][211] fp32.  Each image serves both kinds of read:
//   row operand          S^T = K Q^T, E Q^T, dPd^T = V dO^T
//   transposed operand   O^T += V^T Pd^T, dQ^T += K^T dS^T, dQ^T += E^T dS^T
// The largest image (D = 128) is 2 x 34 816 + 54 016 = 123 648 bytes.
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
        const XfmrSplit s = xfmr_split(r < kXfmrTab ? emb[((size_t)h * kXfmrTab + r) * d + ch] : 0.f);
        hi[i] = __builtin_bit_cast(uint16_t, s.hi);
        lo[i] = __builtin_bit_cast(uint16_t, s.lo);
    }
}

struct XfmrAttn16TrainParams {
    XfmrAttnParams f;  // the fp32 kernel's (emb unused)
    XfmrTab16 tab;
};

struct XfmrAttn16BwdParams {
    XfmrAttnBwdParams b;  // the fp32 kernel's (emb unused)
    XfmrTab16 tab;
};

template <int D>
struct XfmrAttn16TrainLds {
    using R = XfmrAttn16Row<D>;
    static constexpr size_t bytes = (size_t)2 * R::img_bytes + (size_t)kXfmrTQ * kXfmrPosPitch * sizeof(float);
};

// ---------------------------------------------------------------------------------------------------------------------------
// The training forward: xfmr_attn_kernel<D, true>'s statements (dropout factor on the kept probabilities before P V with XfmrDrop's element
// index, L = m + log l per query, zeros on the `out` rows of padded frames, the packed layout) on xfmr_attn16_kernel's products.
// ---------------------------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void xfmr_attn16_train_kernel(const XfmrAttn16TrainParams pp) {
    extern __shared__ __attribute__((aligned(16))) char xfmr16_lds[];
    using R = XfmrAttn16Row<D>;
    constexpr int DP = R::DP, PK = R::PK, NK = R::NK, NM = R::NM, PP = kXfmrPosPitch;
    static_assert(kXfmrKB == 64 && kXfmrTQ == 64, "the staging shares are for 64-key blocks and 256 threads");
    const XfmrAttnParams& p = pp.f;
    char* const kimg = xfmr16_lds;
    char* const vimg = xfmr16_lds + R::img_bytes;
    float* const pos = reinterpret_cast<float*>(xfmr16_lds + 2 * R::img_bytes);
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
    xfmr_attn16_zero(xfmr16_lds, 2 * R::img_bytes, tid);

    bf16x8 qh[NK], ql[NK];
    xfmr_attn16_row_operand<D>(p.qkv + (row0 + (qok ? q : q0)) * F3 + h * D, qok, g, qh, ql);

    XfmrAttn16Stage<D, XfmrAttn16SrcKV> st;
    st.init(tid, p.F, h);
    const int k_lo = max(0, q0 - (kXfmrRel - 1));
    const int k_hi = min(len, q0 + kXfmrTQ + (kXfmrRel - 1));
    st.fetch(p.qkv + (row0 + k_lo) * F3, min(kXfmrKB, k_hi - k_lo));  // in flight during the positional product

    float* const mypos = pos + (wave * 16 + c) * PP;
    const char* const arow = xfmr_attn16_row_ptr<PK>(kimg, c, g);
    xfmr_attn16_pos<D>(kimg, mypos, arow, pp.tab, h, qh, ql, tid, g);
    __syncthreads();
    st.commit(xfmr16_lds);
    __syncthreads();

    const XfmrDrop drop(p.hdr, p.site);
    const unsigned long long e0 = ((unsigned long long)(b * kXfmrHeads + h) * p.T + (qok ? q : 0)) * kXfmrTab;
    float m = -INFINITY, l = 0.f;  // running maximum (-inf: no key yet) and denominator of this lane's query
    f32x4 o[NM];
#pragma unroll
    for (int j = 0; j < NM; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const char* const vtr = xfmr_attn16_tr_ptr<PK>(vimg, c, g);

    for (int kb = k_lo; kb < k_hi; kb += kXfmrKB) {
        const int n = min(kXfmrKB, k_hi - kb);
        const bool more = kb + kXfmrKB < k_hi;
        if (more) st.fetch(p.qkv + (row0 + kb + kXfmrKB) * F3, min(kXfmrKB, k_hi - kb - kXfmrKB));  // the next block travels while this one is multiplied

        f32x4 s[4];
        unsigned valid;
        bool act[2];
        const float alpha = xfmr_attn16_scores<D>(arow, qh, ql, mypos, p.scale, kb, n, q, qw, qok, g, s, valid, act, m, l);
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
            xfmr_attn16_tr_dot<NM, PK, 2 * DP>(vtr + 32 * t * PK, ph, pl, o);
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
// The query-tiled backward: xfmr_attn_bwd_q_kernel's statements.  S^T is recomputed by the forward's own product (xfmr_attn16_rows_dot on the
// same images and operands), so P = exp(S - L) sums to one as the forward's did; dPd^T = V dO^T reads the V image as a row operand;
// dQ^T += K^T dS^T reads the K image transposed, dS split in registers from the accumulators; dQ^T += E^T dS^T sums over the 208 table rows
// in 32-row steps, the table staged through the K image, dS read back as fp32 from the pos rows and split in registers (rows past 198:
// zero operands on both sides).  Delta, the exponential and dS stay fp32; dS and Pd go to the banded fp32 buffers.
// ---------------------------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void xfmr_attn16_bwd_q_kernel(const XfmrAttn16BwdParams pp) {
    extern __shared__ __attribute__((aligned(16))) char xfmr16_lds[];
    using R = XfmrAttn16Row<D>;
    constexpr int DP = R::DP, PK = R::PK, NK = R::NK, NM = R::NM, PP = kXfmrPosPitch;
    const XfmrAttnBwdParams& p = pp.b;
    char* const kimg = xfmr16_lds;
    char* const vimg = xfmr16_lds + R::img_bytes;
    float* const pos = reinterpret_cast<float*>(xfmr16_lds + 2 * R::img_bytes);
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

    xfmr_attn16_zero(xfmr16_lds, 2 * R::img_bytes, tid);

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

    XfmrAttn16Stage<D, XfmrAttn16SrcKV> st;
    st.init(tid, p.F, h);
    const int k_lo = max(0, q0 - (kXfmrRel - 1));
    const int k_hi = min(len, q0 + kXfmrTQ + (kXfmrRel - 1));
    st.fetch(p.qkv + (row0 + k_lo) * F3, min(kXfmrKB, k_hi - k_lo));

    float* const mypos = pos + (wave * 16 + c) * PP;
    const char* const arow = xfmr_attn16_row_ptr<PK>(kimg, c, g);
    xfmr_attn16_pos<D>(kimg, mypos, arow, pp.tab, h, qh, ql, tid, g);
    __syncthreads();
    st.commit(xfmr16_lds);
    __syncthreads();

    f32x4 o[NM];  // dQ^T of this lane's query: rows 16 j + 4 g + i
#pragma unroll
    for (int j = 0; j < NM; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const char* const vrow = xfmr_attn16_row_ptr<PK>(vimg, c, g);
    const char* const ktr = xfmr_attn16_tr_ptr<PK>(kimg, c, g);
    const size_t band = xfmr_band_row(p.lay, row0, b, h, qok ? q : q0, p.T) * kXfmrBand;

    for (int kb = k_lo; kb < k_hi; kb += kXfmrKB) {
        const int n = min(kXfmrKB, k_hi - kb);
        const bool more = kb + kXfmrKB < k_hi;
        if (more) st.fetch(p.qkv + (row0 + kb + kXfmrKB) * F3, min(kXfmrKB, k_hi - kb - kXfmrKB));

        f32x4 ds[4];
        bool act[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) act[t] = xfmr_attn16_step_meets(t, n, kb + 32 * t, qw);
#pragma unroll
        for (int sb = 0; sb < 4; ++sb) {
            ds[sb] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (!act[sb >> 1]) continue;
            const f32x4 s = xfmr_attn16_rows_dot<D>(arow + 16 * sb * PK, qh, ql, f32x4{0.f, 0.f, 0.f, 0.f});
            const f32x4 dp = xfmr_attn16_rows_dot<D>(vrow + 16 * sb * PK, doh, dol, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = kb + 16 * sb + 4 * g + i;
                const int rel = k - q + (kXfmrRel - 1);
                if (xfmr_attn16_in_band(qok, k, kb + n, rel)) {
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
            xfmr_attn16_tr_dot<NM, PK, 2 * DP>(ktr + 32 * t * PK, sh, sl, o);
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
        xfmr_attn16_stage_tab<D>(kimg, pp.tab, h, r0, tid);
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
            xfmr_attn16_tr_dot<NM, PK, 2 * DP>(ktr + 32 * t * PK, sh, sl, o);
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

}  // namespace hificar
