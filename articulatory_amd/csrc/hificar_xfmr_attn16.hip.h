// The bf16x3a forward's attention (hificar_xfmr_set_precision(HIFICAR_PREC_BF16X3A), eval only): xfmr_attn_kernel's plan — one workgroup of
// four waves per (sequence, head, 64 queries), everything transposed so that a query is a lane column, online softmax per 64-key block, keys
// out of band or past the length excluded by a per-element predicate — with its three products as hi.hi + hi.lo + lo.hi on
// v_mfma_f32_16x16x32_bf16 (fp32 accumulation), operands that arrive already split, and the next key block's rows in flight (global ->
// registers) while the current one is multiplied.
//
// Operands.  q | k | v rows are split rows [hi: 3 F bf16 | lo: 3 F bf16] (the q | k | v GEMM's own output pass writes them), the position
// tables are split once at finalize ([8][208][d] hi and lo, rows 199 .. 207 zeros), so every staging step is a 16-byte copy.
//   S^T = K Q^T, P^T = E Q^T   A: lane (c, g) reads channels 32 ks + 8 g .. + 7 of key row 16 sb + c with one ds_read_b128 (hi) and one (lo);
//                              B: this lane's Q[q][32 ks + 8 g .. + 7], hi and lo, loaded once.  Head sizes that are no multiple of 32 (16, 48,
//                              80, 112) pad the LDS key rows with zero channels to the next multiple of 32 (Q's registers are zeros there too).
//   O^T += V^T P^T             32 keys per MFMA: the B operand's slots 8 g + 0 .. 3 are the first 16-key accumulator's registers (keys 4 g + i)
//                              and 8 g + 4 .. 7 the second's (keys 16 + 4 g + i), exponentiated, split and packed — P never goes through LDS;
//                              A: two ds_read_b64_tr_b16 per half of the V rows as staged (keys 4 g .. 4 g + 3 and 16 + 4 g .. of 16 channels).
//                              The transposed read needs EXEC all ones: no lane leaves before the end, and the only branches around it are
//                              wave-uniform (a scalar condition).
// LDS image (bytes): K rows [64][hi: DP bf16 | lo: DP bf16 | 32] — the pitch 4 DP + 32 is 2 (mod 8) 16-byte slots, which puts the 16 lanes of
// every ds_read_b128 lane group ({0-3, 12-15, 20-27}, ...: rows c with chunk g) in 16 different slots of the 256-byte bank row: conflict-free
// (with a 16-byte pad each group is 2-way) — V hi rows [64][PV], V lo rows [64][PV] with PV = 2 D rounded up to an odd multiple of 32: the 8
// rows x 32 bytes a 32-lane half reads transposed fall in 8 different 32-byte slots of the bank row, conflict-free too (0 extra cycles by the
// bank rule for both reads, every head size) — then pos[64][211] fp32 as in xfmr_attn_kernel (its skewed ds_read_b32 is 2-way, as there).
// The order of every sum depends on the query's position and the sequence's length only.
#pragma once
#include "hificar_xfmr_kernels.hip.h"

namespace hificar {

constexpr int kXfmrTabPad = 208;  // rows of one head's split table: 13 tiles of 16, rows 199 .. 207 zeros

struct XfmrAttn16Params {
    const char* qkv;         // [B T][12 F bytes]: split rows of q | k | v, each [head][d]
    const uint16_t* emb_hi;  // [8][208][d] bf16
    const uint16_t* emb_lo;
    const int* lengths;      // device, or null
    char* out;               // [B T][4 F bytes]: split rows, [head][d]
    int T, F;
    float scale;             // 1 / sqrt(d)
};

template <int D>
struct XfmrAttn16Lds {
    static constexpr int DP = (D + 31) / 32 * 32;                 // channels of an LDS key row
    static constexpr int PK = 4 * DP + 32;                        // bytes per key row (hi | lo | pad): 2 (mod 8) 16-byte slots
    static constexpr int PV = 2 * D + ((D / 16) % 2 ? 0 : 32);    // bytes per V row of one half: an odd multiple of 32
    static constexpr int k_bytes = kXfmrKB * PK, v_bytes = kXfmrKB * PV;
    static constexpr size_t bytes = (size_t)k_bytes + 2 * v_bytes + (size_t)kXfmrTQ * kXfmrPosPitch * sizeof(float);
};

typedef short xfmr_s16x4 __attribute__((ext_vector_type(4)));

// 16 channels x (keys 4 g .. 4 g + 3 and 16 + 4 g .. + 3) of a V image as the A operand; `a`: this lane's address of the first block
template <int PV>
__device__ __forceinline__ bf16x8 xfmr_attn16_vfrag(const char* a) {
    typedef __attribute__((address_space(3))) xfmr_s16x4* lds_ptr;
    const xfmr_s16x4 x0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(a));
    const xfmr_s16x4 x1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(a + 16 * PV));
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(x0, x1, 0, 1, 2, 3, 4, 5, 6, 7));
}

// acc += A B with both operands split: the two cross terms, then hi . hi
__device__ __forceinline__ f32x4 xfmr_attn16_mfma3(bf16x8 ah, bf16x8 al, bf16x8 bh, bf16x8 bl, f32x4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, acc, 0, 0, 0);
}

template <int D>
__global__ __launch_bounds__(256) void xfmr_attn16_kernel(const XfmrAttn16Params p) {
    extern __shared__ __attribute__((aligned(16))) char xfmr16_lds[];
    using L = XfmrAttn16Lds<D>;
    constexpr int DP = L::DP, PK = L::PK, PV = L::PV, NK = DP / 32, NM = D / 16, PP = kXfmrPosPitch;
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
    for (int i = tid; i < L::k_bytes / 16; i += 256) *reinterpret_cast<uint4*>(kimg + 16 * i) = make_uint4(0u, 0u, 0u, 0u);

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

    // positional logits of the wave's 16 queries: pos[16 wave + c][r] = Q[q] . E[r], the table staged through the key rows
    float* const mypos = pos + (wave * 16 + c) * PP;
    const char* const arow = kimg + c * PK + 16 * g;  // row c of a 16-row step, this lane's 8 channels of k-step 0
    for (int r0 = 0; r0 < kXfmrTabPad; r0 += kXfmrKB) {
        __syncthreads();
        for (int u = tid; u < kXfmrKB * 2 * CPR; u += 256) {
            const int r = u / (2 * CPR), w = u - r * (2 * CPR), half = w / CPR, ch = w - half * CPR;
            uint4 x = make_uint4(0u, 0u, 0u, 0u);
            if (r0 + r < kXfmrTabPad) x = *reinterpret_cast<const uint4*>((half ? p.emb_lo : p.emb_hi) + ((size_t)h * kXfmrTabPad + r0 + r) * D + 8 * ch);
            *reinterpret_cast<uint4*>(kimg + r * PK + half * 2 * DP + 16 * ch) = x;
        }
        __syncthreads();
#pragma unroll
        for (int sb = 0; sb < 4; ++sb) {
            if (r0 + 16 * sb >= kXfmrTabPad) continue;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const char* a = arow + 16 * sb * PK;
#pragma unroll
            for (int ks = 0; ks < NK; ++ks)
                acc = xfmr_attn16_mfma3(*reinterpret_cast<const bf16x8*>(a + 64 * ks), *reinterpret_cast<const bf16x8*>(a + 2 * DP + 64 * ks), qh[ks], ql[ks], acc);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = r0 + 16 * sb + 4 * g + i;
                if (r < kXfmrTab) mypos[r] = acc[i];
            }
        }
    }
    __syncthreads();
    commit();
    __syncthreads();

    float m = -INFINITY, l = 0.f;  // running maximum (-inf: no key yet) and denominator of this lane's query
    f32x4 o[NM];
#pragma unroll
    for (int j = 0; j < NM; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // this lane's address in the V hi image for the transposed read of keys 4 g .. 4 g + 3, channels 0 .. 15: row 4 g + (c >> 2), channels 4 (c & 3) ..
    const char* const vrow = vimg + (4 * g + (c >> 2)) * PV + 8 * (c & 3);

    for (int kb = k_lo; kb < k_hi; kb += kXfmrKB) {
        const int n = min(kXfmrKB, k_hi - kb);
        const bool more = kb + kXfmrKB < k_hi;
        if (more) fetch(kb + kXfmrKB, min(kXfmrKB, k_hi - kb - kXfmrKB));  // the next block's rows travel while this one is multiplied

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
#pragma unroll
        for (int j = 0; j < NM; ++j) o[j] *= alpha;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            if (!act[t]) continue;
            bf16x8 ph, pl;  // slots 0 .. 3: keys 32 t + 4 g + i; slots 4 .. 7: keys 32 t + 16 + 4 g + i
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float x = s[2 * t + (e >> 2)][e & 3];
                ph[e] = (__bf16)x;
                pl[e] = (__bf16)(x - (float)ph[e]);
            }
            const char* a = vrow + 32 * t * PV;
#pragma unroll
            for (int j = 0; j < NM; ++j)
                o[j] = xfmr_attn16_mfma3(xfmr_attn16_vfrag<PV>(a + 32 * j), xfmr_attn16_vfrag<PV>(a + L::v_bytes + 32 * j), ph, pl, o[j]);
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

template <int D>
static hipError_t xfmr_attn16_launch_one(const XfmrAttn16Params& p, dim3 grid, hipStream_t stream) {
    hipLaunchKernelGGL((xfmr_attn16_kernel<D>), grid, dim3(256), XfmrAttn16Lds<D>::bytes, stream, p);
    return hipGetLastError();
}

static hipError_t xfmr_attn16_attr_all() {
    hipError_t e;
    if ((e = xfmr_attn16_attr<16>()) != hipSuccess) return e;
    if ((e = xfmr_attn16_attr<32>()) != hipSuccess) return e;
    if ((e = xfmr_attn16_attr<48>()) != hipSuccess) return e;
    if ((e = xfmr_attn16_attr<64>()) != hipSuccess) return e;
    if ((e = xfmr_attn16_attr<80>()) != hipSuccess) return e;
    if ((e = xfmr_attn16_attr<96>()) != hipSuccess) return e;
    if ((e = xfmr_attn16_attr<112>()) != hipSuccess) return e;
    return xfmr_attn16_attr<128>();
}

static hipError_t xfmr_attn16_launch(int d, const XfmrAttn16Params& p, dim3 grid, hipStream_t stream) {
    switch (d) {
        case 16: return xfmr_attn16_launch_one<16>(p, grid, stream);
        case 32: return xfmr_attn16_launch_one<32>(p, grid, stream);
        case 48: return xfmr_attn16_launch_one<48>(p, grid, stream);
        case 64: return xfmr_attn16_launch_one<64>(p, grid, stream);
        case 80: return xfmr_attn16_launch_one<80>(p, grid, stream);
        case 96: return xfmr_attn16_launch_one<96>(p, grid, stream);
        case 112: return xfmr_attn16_launch_one<112>(p, grid, stream);
        case 128: return xfmr_attn16_launch_one<128>(p, grid, stream);
    }
    return hipErrorInvalidValue;
}

}  // namespace hificar
