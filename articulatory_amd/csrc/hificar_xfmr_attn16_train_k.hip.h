// The key-tiled attention kernels of the bf16x3wack training arithmetic (hificar_xfmr_set_train_precision, HIFICAR_PREC_BF16X3WACK):
// xfmr_attn16_bwd_k_kernel (dK, dV) and xfmr_demb16_partial_kernel (the first stage of the position tables' gradient), the plans of
// xfmr_attn_bwd_k_kernel and xfmr_demb_partial_kernel with every product as hi.hi + hi.lo + lo.hi on v_mfma_f32_16x16x32_bf16 with fp32
// accumulation.  Both read the banded fp32 dS / Pd buffers exactly as xfmr_attn16_bwd_q_kernel writes them for bf16x3wa and bf16x3wac: no
// second copy of a band, no workspace of their own.
//
// dK, dV.  One workgroup per (sequence, head, 64 keys), a key is a lane column, the queries within +-99 walked in blocks of 64, 32 queries
// per MFMA: dV^T += dO^T Pd and dK^T += Q^T dS.  A query block's dO and Q rows travel as fp32 in registers (the next block in flight while
// the current one is multiplied) and are split when they are committed to LDS (hi = bf16(x), lo = bf16(x - hi)); they are read as the
// transposed operand with ds_read_b64_tr_b16.  A lane's eight Pd and eight dS values of a 32-query step (queries 4 g + i and 16 + 4 g + i
// of the step, this lane's key) are loaded from the bands before the block's products and split in registers.
//
// dE.  partial[chunk][h][r][d] = sum over the chunk's 256 rows of dS[row][r] Q[row][d], the rows in blocks of 64, 32 rows per MFMA.  The
// contraction runs over rows, so BOTH operands are read transposed: the dS block is staged split as [64][hi: 208 | lo: 208] bf16, the Q rows
// as in the other kernel.  Wave w owns the table-row tiles w, w + 4, w + 8 (and 12: wave 0), as in the fp32 kernel.
//
// LDS images (bytes).  dO, Q rows: the common row image.  dS rows: [64][hi: 416 | lo: 416 | 96].  Both pitches are 32 or 160 (mod 256):
// conflict-free transposed reads by the bank rule at every head size.  The largest images (D = 128): 69 632 bytes (dK, dV) and 94 208
// bytes (dE).
//
// The order of every sum depends on the key's (table row's) position and the sequence's length only.  Rows past a block's count, padded
// frames and padded channels are zero operands on the staged side, never read from memory; a band entry is read only where the query-tiled
// kernel wrote it (both frames inside the sequence, the key in the query's band).
#pragma once
#include "hificar_xfmr_attn16_train.hip.h"

namespace hificar {

constexpr int kXfmrEmb16Pitch = 4 * kXfmrEmbPitch + 96;  // bytes per staged dS row: hi | lo | pad; 928 = 160 (mod 256)

template <int D>
struct XfmrAttn16BwdKLds {
    static constexpr size_t bytes = (size_t)2 * XfmrAttn16Row<D>::img_bytes;  // dO rows, Q rows
};

template <int D>
struct XfmrEmb16Lds {
    static constexpr int ds_bytes = 64 * kXfmrEmb16Pitch;
    static constexpr size_t bytes = (size_t)ds_bytes + XfmrAttn16Row<D>::img_bytes;  // dS block, Q rows
};

template <int D>
__global__ __launch_bounds__(256) void xfmr_attn16_bwd_k_kernel(const XfmrAttnBwdParams p) {
    extern __shared__ __attribute__((aligned(16))) char xfmr16_lds[];
    using R = XfmrAttn16Row<D>;
    constexpr int DP = R::DP, PK = R::PK, NM = R::NM;
    static_assert(kXfmrKB == 64, "the staging shares are for 64-query blocks and 256 threads");
    char* const doimg = xfmr16_lds;
    char* const qimg = xfmr16_lds + R::img_bytes;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
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

    // the padded channels of both images are zeros from here on: the staging never writes them
    xfmr_attn16_zero(xfmr16_lds, 2 * R::img_bytes, tid);

    XfmrAttn16Stage<D, XfmrAttn16SrcDoQ> st;
    st.init(tid, p.F, h);
    const int q_lo = max(0, k0 - (kXfmrRel - 1));
    const int q_hi = min(len, k0 + kXfmrKB + (kXfmrRel - 1));
    st.fetch(p.dout + (row0 + q_lo) * p.F, p.qkv + (row0 + q_lo) * F3, min(kXfmrKB, q_hi - q_lo));
    __syncthreads();
    st.commit(xfmr16_lds);
    __syncthreads();

    f32x4 dv[NM], dk[NM];
#pragma unroll
    for (int j = 0; j < NM; ++j) dv[j] = dk[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const char* const dotr = xfmr_attn16_tr_ptr<PK>(doimg, c, g);
    const char* const qtr = xfmr_attn16_tr_ptr<PK>(qimg, c, g);

    for (int qb = q_lo; qb < q_hi; qb += kXfmrKB) {
        const int n = min(kXfmrKB, q_hi - qb);
        const bool more = qb + kXfmrKB < q_hi;
        if (more) st.fetch(p.dout + (row0 + qb + kXfmrKB) * p.F, p.qkv + (row0 + qb + kXfmrKB) * F3, min(kXfmrKB, q_hi - qb - kXfmrKB));

        // this lane's band entries of the block: slot e of step t is query qb + 32 t + 16 (e >> 2) + 4 g + (e & 3)
        f32x4 pv[2][2], sv[2][2];
        bool act[2];  // (wave-uniform) the 32-query step meets the band of the wave's keys kw .. kw + 15
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int q32 = qb + 32 * t;
            act[t] = xfmr_attn16_step_meets(t, n, q32, kw);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                pv[t][u] = sv[t][u] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (!act[t]) continue;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int q = q32 + 16 * u + 4 * g + i;
                    const int rel = k - q + (kXfmrRel - 1);
                    if (xfmr_attn16_in_band(kok, q, qb + n, rel)) {
                        const size_t e = xfmr_band_row(p.lay, row0, b, h, q, p.T) * kXfmrBand + rel;
                        pv[t][u][i] = p.pd[e];
                        sv[t][u][i] = p.ds[e];
                    }
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            if (!act[t]) continue;
            bf16x8 ph, pl, sh, sl;
            xfmr_split_b(pv[t][0], pv[t][1], ph, pl);
            xfmr_split_b(sv[t][0], sv[t][1], sh, sl);
            xfmr_attn16_tr_dot<NM, PK, 2 * DP>(dotr + 32 * t * PK, ph, pl, dv);
            xfmr_attn16_tr_dot<NM, PK, 2 * DP>(qtr + 32 * t * PK, sh, sl, dk);
        }
        if (!more) break;
        __syncthreads();  // every wave has read this block
        st.commit(xfmr16_lds);
        __syncthreads();
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

typedef __bf16 xfmr_bf16x4 __attribute__((ext_vector_type(4)));

template <int D>
__global__ __launch_bounds__(256) void xfmr_demb16_partial_kernel(const float* __restrict__ qkv, const float* __restrict__ ds, float* __restrict__ partial,
                                                                  int M, int T, int F, const BigruTapeHeader* hdr, const int* __restrict__ tape_lens,
                                                                  const XfmrLayout lay) {
    extern __shared__ __attribute__((aligned(16))) char xfmr16_lds[];
    using R = XfmrAttn16Row<D>;
    using E = XfmrEmb16Lds<D>;
    constexpr int DP = R::DP, PK = R::PK, NM = R::NM, PS = kXfmrEmb16Pitch, NT = kXfmrEmbPitch / 16;
    static_assert(kXfmrBand % 4 == 0 && kXfmrBand <= kXfmrEmbPitch && kXfmrEmbRows % 64 == 0, "the staging of a dS block");
    char* const dimg = xfmr16_lds;
    char* const qimg = xfmr16_lds + E::ds_bytes;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, g = lane >> 4;
    const int chunk = blockIdx.x, h = blockIdx.y;
    const size_t F3 = (size_t)3 * F;
    const int* const lens = bigru_tape_lens(hdr, tape_lens);

    // columns 200 .. 207 of the dS rows and the padded channels of the Q rows are zeros from here on: the staging never writes them
    xfmr_attn16_zero(xfmr16_lds, (int)E::bytes, tid);

    f32x4 acc[4][NM];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int j = 0; j < NM; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const char* const atr = xfmr_attn16_tr_ptr<PS>(dimg, c, g);
    const char* const btr = xfmr_attn16_tr_ptr<PK>(qimg, c, g);

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
        __syncthreads();  // every wave has read the block before
        for (int i = tid; i < 64 * (D / 8); i += 256) {
            const int rr = i / (D / 8), v = i - rr * (D / 8);
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
            if (rr < n && xfmr_row_valid(lay, lens, r0 + rr, T)) {
                const float* s = qkv + (size_t)(r0 + rr) * F3 + h * D + 8 * v;
                x = *reinterpret_cast<const float4*>(s);
                y = *reinterpret_cast<const float4*>(s + 4);
            }
            bf16x8 hi, lo;
            xfmr_split8(x, y, hi, lo);
            *reinterpret_cast<bf16x8*>(qimg + rr * PK + 16 * v) = hi;
            *reinterpret_cast<bf16x8*>(qimg + rr * PK + 2 * DP + 16 * v) = lo;
        }
        for (int i = tid; i < 64 * (kXfmrBand / 4); i += 256) {
            const int rr = i / (kXfmrBand / 4), v = i - rr * (kXfmrBand / 4);
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (rr < n && xfmr_row_valid(lay, lens, r0 + rr, T)) {  // (entry 199 of a row is a written zero)
                const int row = r0 + rr, bb = row / T, t = row - bb * T;
                const size_t band = lay.pad_row ? (size_t)row * kXfmrHeads + h : ((size_t)bb * kXfmrHeads + h) * T + t;
                x = *reinterpret_cast<const float4*>(ds + band * kXfmrBand + 4 * v);
            }
            const float v4[4] = {x.x, x.y, x.z, x.w};
            xfmr_bf16x4 hi, lo;
            xfmr_split_n(v4, hi, lo);
            *reinterpret_cast<xfmr_bf16x4*>(dimg + rr * PS + 8 * v) = hi;
            *reinterpret_cast<xfmr_bf16x4*>(dimg + rr * PS + 2 * kXfmrEmbPitch + 8 * v) = lo;
        }
        __syncthreads();
        // (the transposed product with its B fragments hoisted out of the table-row tiles: xfmr_attn16_tr_dot's statement, the A operand
        // on the dS pitch)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (32 * s >= n) continue;  // (the whole workgroup)
            bf16x8 bh[NM], bl[NM];
#pragma unroll
            for (int j = 0; j < NM; ++j) {
                bh[j] = xfmr_attn16_vfrag<PK>(btr + 32 * s * PK + 32 * j);
                bl[j] = xfmr_attn16_vfrag<PK>(btr + 32 * s * PK + 2 * DP + 32 * j);
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int rt = wave + 4 * t;
                if (rt >= NT) continue;  // (wave-uniform)
                const bf16x8 ah = xfmr_attn16_vfrag<PS>(atr + 32 * s * PS + 32 * rt);
                const bf16x8 al = xfmr_attn16_vfrag<PS>(atr + 32 * s * PS + 2 * kXfmrEmbPitch + 32 * rt);
#pragma unroll
                for (int j = 0; j < NM; ++j) acc[t][j] = xfmr_attn16_mfma3(ah, al, bh[j], bl[j], acc[t][j]);
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
            if (rt >= NT || r >= kXfmrTab) continue;
#pragma unroll
            for (int j = 0; j < NM; ++j) dst[(size_t)r * D + 16 * j + c] = acc[t][j][i];
        }
    }
}

template <int D>
static hipError_t xfmr_attn16_train_k_attr() {
    static_assert(XfmrAttn16BwdKLds<D>::bytes <= 160 * 1024 && XfmrEmb16Lds<D>::bytes <= 160 * 1024, "the key-tiled kernels' LDS");
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&xfmr_attn16_bwd_k_kernel<D>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)XfmrAttn16BwdKLds<D>::bytes);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&xfmr_demb16_partial_kernel<D>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)XfmrEmb16Lds<D>::bytes);
}

}  // namespace hificar
