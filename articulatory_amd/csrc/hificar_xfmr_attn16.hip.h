// The bf16x3a forward's attention (hificar_xfmr_set_precision(HIFICAR_PREC_BF16X3A), eval only): xfmr_attn_kernel's plan — one workgroup of
// four waves per (sequence, head, 64 queries), everything transposed so that a query is a lane column, online softmax per 64-key block, keys
// out of band or past the length excluded by a per-element predicate — on the building blocks of hificar_xfmr_attn16_common.hip.h, with
// operands that arrive already split.
//
// Operands.  q | k | v rows are split rows [hi: 3 F bf16 | lo: 3 F bf16] (the q | k | v GEMM's own output pass writes them), the position
// tables are split once at finalize ([8][208][d] hi and lo, rows 199 .. 207 zeros), so every staging step is a 16-byte copy.
//   S^T = K Q^T, P^T = E Q^T   row operand: the K image; B: this lane's Q[q][32 ks + 8 g .. + 7], hi and lo, loaded once.  Head sizes that
//                              are no multiple of 32 (16, 48, 80, 112) have zero channels up to DP (Q's registers are zeros there too).
//   O^T += V^T P^T             transposed operand: the V rows as staged, P exponentiated, split and packed in registers.
// LDS image (bytes): K rows as the common row image; V hi rows [64][PV], V lo rows [64][PV] with PV = 2 D rounded up to an odd multiple of
// 32: the 8 rows x 32 bytes a 32-lane half reads transposed fall in 8 different 32-byte slots of the bank row, conflict-free too (0 extra
// cycles by the bank rule for both reads, every head size) — then pos[64][211] fp32 as in xfmr_attn_kernel (its skewed ds_read_b32 is 2-way,
// as there).
// The order of every sum depends on the query's position and the sequence's length only.
#pragma once
#include "hificar_xfmr_attn16_common.hip.h"

namespace hificar {

struct XfmrAttn16Params {
    const char* qkv;         // [B T][12 F bytes]: split rows of q | k | v, each [head][d]
    XfmrTab16 tab;
    const int* lengths;      // device, or null
    char* out;               // [B T][4 F bytes]: split rows, [head][d]
    int T, F;
    float scale;             // 1 / sqrt(d)
};

template <int D>
struct XfmrAttn16Lds {
    using R = XfmrAttn16Row<D>;
    static constexpr int PV = 2 * D + ((D / 16) % 2 ? 0 : 32);    // bytes per V row of one half: an odd multiple of 32
    static constexpr int k_bytes = R::img_bytes, v_bytes = kXfmrKB * PV;
    static constexpr size_t bytes = (size_t)k_bytes + 2 * v_bytes + (size_t)kXfmrTQ * kXfmrPosPitch * sizeof(float);
};

template <int D>
__global__ __launch_bounds__(256) void xfmr_attn16_kernel(const XfmrAttn16Params p) {
    extern __shared__ __attribute__((aligned(16))) char xfmr16_lds[];
    using L = XfmrAttn16Lds<D>;
    using R = XfmrAttn16Row<D>;
    constexpr int DP = R::DP, PK = R::PK, PV = L::PV, NK = R::NK, NM = R::NM, PP = kXfmrPosPitch;
    constexpr int CPR = D / 8;  // 16-byte pieces per half of a head's row
    static_assert(kXfmrKB == 64 && kXfmrTQ == 64, "the staging shares below are for 64-key blocks and 256 threads");
    char* const kimg = xfmr16_lds;
    char* const vimg = xfmr16_lds + L::k_bytes;  // hi, then lo
    float* const pos = reinterpret_cast<float*>(xfmr16_lds + L::k_bytes + 2 * L::v_bytes);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, g = lane >> 4;
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * kXfmrTQ;
    const int len = p.lengths ? min(max(p.lengths[b], 0), p.T) : p.T;
    if (q0 >= len) return;  // (the whole workgroup: no barrier has been reached)
    const size_t row0 = (size_t)b * p.T;
    const size_t RB = (size_t)12 * p.F;  // bytes per q | k | v row
    const int qw = q0 + wave * 16, q = qw + c;
    const bool qok = q < len;

    // the padded channels of the key rows are zeros from here on: the staging never writes them
    xfmr_attn16_zero(kimg, L::k_bytes, tid);

    // this lane's B operands of S^T and the positional product: Q[q][32 ks + 8 g .. + 7], hi and lo (zeros: padded query, padded channel)
    bf16x8 qh[NK], ql[NK];
    {
        const char* qrow = p.qkv + (row0 + (qok ? q : q0)) * RB + 2 * (h * D);
#pragma unroll
        for (int ks = 0; ks < NK; ++ks) {
            uint4 vh = make_uint4(0u, 0u, 0u, 0u), vl = vh;
            if (qok && 32 * ks + 8 * g < D) {
                vh = *reinterpret_cast<const uint4*>(qrow + 2 * (32 * ks + 8 * g));
                vl = *reinterpret_cast<const uint4*>(qrow + RB / 2 + 2 * (32 * ks + 8 * g));
            }
            qh[ks] = __builtin_bit_cast(bf16x8, vh);
            ql[ks] = __builtin_bit_cast(bf16x8, vl);
        }
    }

    // The operands arrive split, so this staging copies 16-byte pieces into two pitches (PK and PV): a small thing of its own, not
    // XfmrAttn16Stage, which splits fp32 pieces into two row images.
    // This thread's share of a 64-key block: CPR pieces of 16 bytes.  Piece u = tid + 256 i is piece (u mod 4 CPR) of key row u / (4 CPR); a row's
    // pieces are K hi, K lo, V hi, V lo, CPR each.  Source and destination offsets are the same for every block.
    int st_row[CPR], st_src[CPR], st_dst[CPR];
#pragma unroll
    for (int i = 0; i < CPR; ++i) {
        const int u = tid + 256 * i, r = u / (4 * CPR), w = u - r * (4 * CPR), part = w / CPR, ch = w - part * CPR;
        st_row[i] = r;
        st_src[i] = r * (int)RB + (part & 1) * (int)(RB / 2) + 2 * (((part >> 1) + 1) * p.F + h * D + 8 * ch);
        st_dst[i] = part < 2 ? r * PK + (part & 1) * 2 * DP + 16 * ch : L::k_bytes + (part & 1) * L::v_bytes + r * PV + 16 * ch;
    }
    uint4 st[CPR];
    // rows at or past n are zeros, never copied: the workspace rows past a sequence's length hold whatever was there
    auto fetch = [&](int kb, int n) {
        const char* base = p.qkv + (row0 + kb) * RB;
#pragma unroll
        for (int i = 0; i < CPR; ++i) {
            st[i] = make_uint4(0u, 0u, 0u, 0u);
            if (st_row[i] < n) st[i] = *reinterpret_cast<const uint4*>(base + st_src[i]);
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int i = 0; i < CPR; ++i) *reinterpret_cast<uint4*>(xfmr16_lds + st_dst[i]) = st[i];
    };

    const int k_lo = max(0, q0 - (kXfmrRel - 1));
    const int k_hi = min(len, q0 + kXfmrTQ + (kXfmrRel - 1));
    fetch(k_lo, min(kXfmrKB, k_hi - k_lo));  // in flight during the positional product

    float* const mypos = pos + (wave * 16 + c) * PP;
    const char* const arow = xfmr_attn16_row_ptr<PK>(kimg, c, g);
    xfmr_attn16_pos<D>(kimg, mypos, arow, p.tab, h, qh, ql, tid, g);
    __syncthreads();
    commit();
    __syncthreads();

    float m = -INFINITY, l = 0.f;  // running maximum (-inf: no key yet) and denominator of this lane's query
    f32x4 o[NM];
#pragma unroll
    for (int j = 0; j < NM; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const char* const vrow = xfmr_attn16_tr_ptr<PV>(vimg, c, g);

    for (int kb = k_lo; kb < k_hi; kb += kXfmrKB) {
        const int n = min(kXfmrKB, k_hi - kb);
        const bool more = kb + kXfmrKB < k_hi;
        if (more) fetch(kb + kXfmrKB, min(kXfmrKB, k_hi - kb - kXfmrKB));  // the next block's rows travel while this one is multiplied

        f32x4 s[4];
        unsigned valid;
        bool act[2];
        const float alpha = xfmr_attn16_scores<D>(arow, qh, ql, mypos, p.scale, kb, n, q, qw, qok, g, s, valid, act, m, l);
#pragma unroll
        for (int j = 0; j < NM; ++j) o[j] *= alpha;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            if (!act[t]) continue;
            bf16x8 ph, pl;
            xfmr_split_b(s[2 * t], s[2 * t + 1], ph, pl);
            xfmr_attn16_tr_dot<NM, PV, L::v_bytes>(vrow + 32 * t * PV, ph, pl, o);
        }
        if (!more) break;
        __syncthreads();  // every wave has read this block
        commit();
        __syncthreads();
    }
    const float inv = qok ? 1.f / l : 0.f;  // (l >= 1: the query's own key is in its band)
    char* const orow = p.out + (row0 + (qok ? q : q0)) * (size_t)p.F * 4;  // (qok is shared by the lanes of a column)
#pragma unroll
    for (int j = 0; j < NM; ++j)
        xfmr_store_split(orow, p.F, h * D + 16 * j + 4 * g, g & 1, 16, o[j][0] * inv, o[j][1] * inv, o[j][2] * inv, o[j][3] * inv, qok);
}

template <int D>
static hipError_t xfmr_attn16_attr() {
    static_assert(XfmrAttn16Lds<D>::bytes <= 160 * 1024, "one workgroup per CU");
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&xfmr_attn16_kernel<D>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)XfmrAttn16Lds<D>::bytes);
}

}  // namespace hificar
