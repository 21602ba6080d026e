// The HuBERT encoder's bf16x3a attention (hificar_hubert_set_precision(HIFICAR_PREC_BF16X3A), inference only): hubert_attn_kernel's plan — one
// workgroup of four waves per (sequence, head, 64 queries), everything transposed so that a query is a lane column, online softmax per
// 64-key block over ALL the utterance's keys — on the building blocks of hificar_xfmr_attn16_common.hip.h.  It is xfmr_attn16_kernel without
// band, table and `pos` region: the score helper's BAND = false form.
//
// Operands.  q | k | v rows arrive as split rows [hi: 3 F bf16 | lo: 3 F bf16] (the q | k | v GEMM's own output pass writes them), so every
// staging step is a 16-byte copy; the next 64-key block travels global -> registers while the current one is multiplied.
//   S^T = K Q^T      row operand: the K image; B: this lane's Q[q][32 ks + 8 g .. + 7], hi and lo, loaded once
//   O^T += V^T P^T   transposed operand (ds_read_b64_tr_b16): the V rows as staged; P exponentiated, split and packed in registers, never
//                    in LDS; the row sum is taken from the fp32 exponentials
// Keys past the length are written to LDS as zeros, never copied, and excluded by predicate (weight 0, no part in the maximum); queries
// past it are computed on zero operands and not stored.  The only early exit is the whole workgroup's at q0 >= len, so EXEC is all ones at
// every transposed read; the branches around one depend on the block's key count alone (workgroup-uniform).
// LDS image (bytes): K rows as the common row image [64][PK = 4 DP + 32]; V hi rows [64][PV], V lo rows [64][PV], PV = 2 D rounded up to an
// odd multiple of 32 (XfmrAttn16Lds<D>::PV).  The bank-rule argument is xfmr_attn16_kernel's: PK is 2 (mod 8) 16-byte slots, so the 16 lanes
// of a ds_read_b128 lane group fall in 16 different slots of the 256-byte bank row; PV is an odd multiple of 32 bytes, so the 8 rows x 32
// bytes a 32-lane half reads transposed start at 8 different multiples of 32 in the bank row.  D = 64: PK = 288, PV = 160, 38 912 bytes.
// The order of every sum depends on the query's position and the utterance's length only.
#pragma once
#include "hificar_xfmr_attn16.hip.h"

namespace hificar {

struct HubertAttn16Params {
    const char* qkv;     // [B T][12 F bytes]: split rows of q | k | v, each [head][d]
    const int* lengths;  // device, or null
    char* out;           // [B T][4 F bytes]: split rows, [head][d]
    int T, F;
    float scale;         // 1 / sqrt(d)
};

template <int D>
struct HubertAttn16Lds {
    using X = XfmrAttn16Lds<D>;
    static constexpr size_t bytes = (size_t)X::k_bytes + 2 * X::v_bytes;
};

template <int D>
__global__ __launch_bounds__(256) void hubert_attn16_kernel(const HubertAttn16Params p) {
    extern __shared__ __attribute__((aligned(16))) char hubert16_lds[];
    using L = XfmrAttn16Lds<D>;
    using R = XfmrAttn16Row<D>;
    constexpr int DP = R::DP, PK = R::PK, PV = L::PV, NK = R::NK, NM = R::NM;
    constexpr int CPR = D / 8;  // 16-byte pieces per half of a head's row
    static_assert(kXfmrKB == 64 && kXfmrTQ == 64, "the staging shares below are for 64-key blocks and 256 threads");
    static_assert((64 * 4 * CPR) % 256 == 0, "a block's pieces divide among 256 threads");
    char* const kimg = hubert16_lds;
    char* const vimg = hubert16_lds + L::k_bytes;  // hi, then lo
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

    // this lane's B operands of S^T: Q[q][32 ks + 8 g .. + 7], hi and lo (zeros: padded query, padded channel)
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
        for (int i = 0; i < CPR; ++i) *reinterpret_cast<uint4*>(hubert16_lds + st_dst[i]) = st[i];
    };

    fetch(0, min(kXfmrKB, len));
    __syncthreads();  // the zeroing is done before a piece lands on it
    commit();
    __syncthreads();

    float m = -INFINITY, l = 0.f;  // running maximum (-inf: no key yet) and denominator of this lane's query
    f32x4 o[NM];
#pragma unroll
    for (int j = 0; j < NM; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const char* const arow = xfmr_attn16_row_ptr<PK>(kimg, c, g);
    const char* const vrow = xfmr_attn16_tr_ptr<PV>(vimg, c, g);

    for (int kb = 0; kb < len; kb += kXfmrKB) {
        const int n = min(kXfmrKB, len - kb);
        const bool more = kb + kXfmrKB < len;
        if (more) fetch(kb + kXfmrKB, min(kXfmrKB, len - kb - kXfmrKB));  // the next block's rows travel while this one is multiplied

        f32x4 s[4];
        unsigned valid;
        bool act[2];
        const float alpha = xfmr_attn16_scores<D, false>(arow, qh, ql, nullptr, p.scale, kb, n, q, qw, qok, g, s, valid, act, m, l);
#pragma unroll
        for (int j = 0; j < NM; ++j) o[j] *= alpha;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            if (!act[t]) continue;  // (workgroup-uniform: the block has no key in this half)
            bf16x8 ph, pl;
            xfmr_split_b(s[2 * t], s[2 * t + 1], ph, pl);
            xfmr_attn16_tr_dot<NM, PV, L::v_bytes>(vrow + 32 * t * PV, ph, pl, o);
        }
        if (!more) break;
        __syncthreads();  // every wave has read this block
        commit();
        __syncthreads();
    }
    const float inv = qok ? 1.f / l : 0.f;  // (l >= 1: the query's own key exists)
    char* const orow = p.out + (row0 + (qok ? q : q0)) * (size_t)p.F * 4;  // (qok is shared by the lanes of a column)
#pragma unroll
    for (int j = 0; j < NM; ++j)
        xfmr_store_split(orow, p.F, h * D + 16 * j + 4 * g, g & 1, 16, o[j][0] * inv, o[j][1] * inv, o[j][2] * inv, o[j][3] * inv, qok);
}

template <int D>
static hipError_t hubert_attn16_attr() {
    static_assert(HubertAttn16Lds<D>::bytes <= 160 * 1024, "one workgroup per CU at the least");
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&hubert_attn16_kernel<D>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)HubertAttn16Lds<D>::bytes);
}

}  // namespace hificar
