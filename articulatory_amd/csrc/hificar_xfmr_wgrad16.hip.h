// The weight gradients of the Transformer's bf16x3w training arithmetic (hificar_xfmr_set_train_precision, HIFICAR_PREC_BF16X3W): the
// one-tap GEMM form dW = G^T A (wgrad_gemm_form: the layers wgrad_gemm_kernel runs in fp32) on v_mfma_f32_32x32x16_bf16, three bf16
// products per fp32 product, fp32 accumulation.
//   xfmr_split_rows_t_kernel   fp32 rows [M][C] -> [ceil(M / 8)][C][hi 8 | lo 8] bf16: 32 bytes per (group of 8 rows, channel).  The MFMA sums
//                              over ROWS here, so a lane's 16-byte operand is 8 consecutive rows of one channel: this layout makes it one read.
//                              hi = bf16(x), lo = bf16(x - hi), round to nearest even (xfmr_split_rows_kernel's expression).  Rows past M, rows
//                              of padded frames (ragged tape) and gap rows (packed) are written as zero bits and not read.
//   wgrad_bf16x3_kernel        the GEMM on those rows, wgrad_gemm_kernel's tiling (128 x 128 on 64-row chunks, 128 x 256 on 32-row chunks, chunks
//                              double-buffered through LDS-DMA, the row chunks split over blockIdx.y) and its partial / bias-partial layouts: the
//                              reductions behind it are the fp32 form's.  Fixed summation order, no atomics.
//   xfmr_split_taps_t_kernel   bf16x3wac (HIFICAR_PREC_BF16X3WAC): the A operand of a wide k = 3 conv's weight gradient, run as the one-tap GEMM
//                              dW[co][k C + c] = G^T A3.  fp32 rows [M][C] -> [ceil(M / 8)][3 C][hi 8 | lo 8]: column k C + c of row r holds row
//                              r + k - 1 of channel c, and zero bits where that row lies outside [0, M), is a padded frame or a gap row, or
//                              belongs to another sequence than row r.  Such rows are not read.
// The splits' index arithmetic is plain C++ (HIFICAR_HD): hificar_debug_split_rows_t and hificar_debug_split_taps_t run the same functions on
// the host.
#pragma once
#include "hificar_xfmr_pack16.hip.h"

namespace hificar {

HIFICAR_HD long long split_t_groups(long long M) { return (M + 7) >> 3; }
HIFICAR_HD long long split_t_items(long long M, int C) { return split_t_groups(M) * C; }  // one item: one (group, channel), 32 bytes
HIFICAR_HD long long split_t_bytes(long long M, int C) { return split_t_items(M, C) * 32; }
// byte offset of the hi value of (row r, channel c); its lo value: + 16
HIFICAR_HD long long split_t_offset(int C, long long r, int c) { return ((r >> 3) * C + c) * 32 + (r & 7) * 2; }

HIFICAR_HD void split_t_pair(float v, uint16_t* hi, uint16_t* lo) {
#if defined(__HIP_DEVICE_COMPILE__)
    const __bf16 h = (__bf16)v, l = (__bf16)(v - (float)h);
    memcpy(hi, &h, 2);
    memcpy(lo, &l, 2);
#else
    *hi = pack16_bf16(v);
    *lo = pack16_bf16(v - pack16_f32(*hi));
#endif
}

// one item: reads up to 8 floats of one column, writes 32 adjacent bytes.  valid(r): row r < M is a frame of its sequence
template <typename V>
HIFICAR_HD void split_t_item(const float* x, char* dst, long long M, int C, long long i, V valid) {
    const long long gi = i / C;
    const int c = (int)(i - gi * C);
    alignas(16) uint16_t v[16];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < 8; ++j) {
        const long long r = gi * 8 + j;
        v[j] = v[8 + j] = 0;
        if (r < M && valid(r)) split_t_pair(x[r * C + c], &v[j], &v[8 + j]);
    }
    memcpy(dst + split_t_offset(C, gi * 8, c), v, 32);
}

// The tap-column split.  One item: one (group of 8 rows, channel) for all three taps: reads the channel's rows 8 gi - 1 .. 8 gi + 8 once (the
// valid ones among them), writes three runs of 32 bytes, C columns apart.  Tseq: rows per sequence (dense, ragged: T; packed: anything above
// M — the gap rows are the sequences' ends).  valid(s): row s < M is a frame of its sequence.
HIFICAR_HD long long split_t3_items(long long M, int C) { return split_t_groups(M) * C; }
HIFICAR_HD long long split_t3_bytes(long long M, int C) { return split_t_bytes(M, 3 * C); }

template <typename V>
HIFICAR_HD void split_t3_item(const float* x, char* dst, long long M, int C, long long Tseq, long long i, V valid) {
    const long long gi = i / C;
    const int c = (int)(i - gi * C);
    const long long r0 = gi * 8;
    uint16_t hi[10], lo[10];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < 10; ++j) {
        const long long s = r0 - 1 + j;
        hi[j] = lo[j] = 0;
        if (s >= 0 && s < M && valid(s)) split_t_pair(x[s * C + c], &hi[j], &lo[j]);
    }
    const long long t0 = r0 % Tseq;  // the frame row r0 is in its sequence
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 3; ++k) {
        alignas(16) uint16_t v[16];
        long long t = t0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int j = 0; j < 8; ++j) {
            // the frame in front of a sequence's first and the one behind its last are another sequence's (or nobody's)
            const bool in = !(k == 0 && t == 0) && !(k == 2 && t == Tseq - 1);
            v[j] = in ? hi[j + k] : (uint16_t)0;
            v[8 + j] = in ? lo[j + k] : (uint16_t)0;
            if (++t == Tseq) t = 0;
        }
        memcpy(dst + split_t_offset(3 * C, r0, k * C + c), v, 32);
    }
}

#if defined(__HIPCC__)
// hdr = null: `tape_lens` holds as it stands (null: dense) — the debug entry
__global__ __launch_bounds__(256) void xfmr_split_rows_t_kernel(const float* __restrict__ x, char* __restrict__ dst, long long M, int C,
                                                                const BigruTapeHeader* hdr, const int* __restrict__ tape_lens, int T, const XfmrLayout lay) {
    const int* const lens = hdr ? bigru_tape_lens(hdr, tape_lens) : tape_lens;
    const long long n = split_t_items(M, C);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        split_t_item(x, dst, M, C, i, [&](long long r) { return xfmr_row_valid(lay, lens, r, T); });
}

// hdr = null: as above.  T: the rows of a sequence (packed: not used)
__global__ __launch_bounds__(256) void xfmr_split_taps_t_kernel(const float* __restrict__ x, char* __restrict__ dst, long long M, int C,
                                                                const BigruTapeHeader* hdr, const int* __restrict__ tape_lens, int T, const XfmrLayout lay) {
    const int* const lens = hdr ? bigru_tape_lens(hdr, tape_lens) : tape_lens;
    const long long n = split_t3_items(M, C), Tseq = lay.pad_row ? M + 8 : T;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        split_t3_item(x, dst, M, C, Tseq, i, [&](long long s) { return xfmr_row_valid(lay, lens, s, T); });
}

struct WgradX3Params {
    const char* g16;  // split rows of G, [groups][gC][32 bytes]
    const char* a16;  // ... and of A, [groups][aC][32 bytes]
    int groups;       // ceil(rows / 8)
    int gC, aC;       // channels of the split buffers: columns at or past them are zeros, never read
    int n_gblk, n_ablk;
    int nsplit;
    float* partial;       // [nsplit][n_gblk * 32][n_ablk * 32]
    float* bias_partial;  // [nsplit][n_gblk * 32], or null
    const char* zeros;    // >= 16 zero bytes
};

// LDS, per buffer: [group of the chunk][32-channel block of the G tile (4)][hi: 32 lanes x 16 B | lo: the same], then the same for the A
// tile's 2 AJ blocks.  One LDS-DMA wave-instruction fills one (group, block) KiB: lanes 0-31 fetch the hi halves of 32 channels, lanes
// 32-63 the lo halves, so a ds_read_b128 of 32 lanes' hi (or lo) fragments is 512 contiguous bytes.  An MFMA's K = 16 rows are two groups:
// lanes 0-31 read group 2 s, lanes 32-63 group 2 s + 1.
template <int AJ, int R>
__global__ __launch_bounds__(256) void wgrad_bf16x3_kernel(const WgradX3Params p) {
    static_assert((AJ == 2 && R == 64) || (AJ == 4 && R == 32), "128 x 128 tile on 64-row chunks, or 128 x 256 on 32-row chunks");
    constexpr int AW = AJ * 64, GPC = R / 8, NBA = 2 * AJ;
    constexpr int g_bytes = GPC * 4 * 1024, buf_bytes = g_bytes + GPC * NBA * 1024;
    extern __shared__ __attribute__((aligned(1024))) char wg16_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, hf = lane >> 5;
    const int at_n = (p.n_ablk + NBA - 1) / NBA;
    const int at = blockIdx.x % at_n, gt = blockIdx.x / at_n;
    const int split = blockIdx.y;
    const int gw = wave >> 1, aw = wave & 1;
    const int nchunks = (p.groups + GPC - 1) / GPC;
    const int c_lo = (int)((long long)nchunks * split / p.nsplit), c_hi = (int)((long long)nchunks * (split + 1) / p.nsplit);
    f32x16 acc[2][AJ];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < AJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // A wave stages block `wave` of the G tile and blocks wave, wave + 4 (AJ = 4) of the A tile, of every group of the chunk: the lane's
    // part of each source address is fixed, the group's is one multiply-add, the LDS offsets are immediates of the unrolled loop.
    // (The chunks are short next to the fp32 form's — 24 MFMAs of 8 passes per K step — so the staging code's own length counts.)
    constexpr int AQ = NBA / 4;
    const int gch = gt * 128 + wave * 32 + li;
    const char* const g_lane = gch < p.gC ? p.g16 + (size_t)gch * 32 + hf * 16 : nullptr;
    const char* a_lane[AQ];
#pragma unroll
    for (int q = 0; q < AQ; ++q) {
        const int ach = at * AW + (wave + 4 * q) * 32 + li;
        a_lane[q] = ach < p.aC ? p.a16 + (size_t)ach * 32 + hf * 16 : nullptr;
    }
    const size_t g_step = (size_t)p.gC * 32, a_step = (size_t)p.aC * 32;  // bytes per group
    auto stage = [&](int c, int b) {
        char* dst = wg16_smem + b * buf_bytes;
#pragma unroll
        for (int gi = 0; gi < GPC; ++gi) {
            const int grp = c * GPC + gi;
            const bool in = grp < p.groups;
            const char* src = in && g_lane ? g_lane + grp * g_step : p.zeros;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(dst + (gi * 4 + wave) * 1024), 16, 0, 0);
#pragma unroll
            for (int q = 0; q < AQ; ++q) {
                src = in && a_lane[q] ? a_lane[q] + grp * a_step : p.zeros;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                 (__attribute__((address_space(3))) void*)(dst + g_bytes + (gi * NBA + wave + 4 * q) * 1024), 16, 0, 0);
            }
        }
    };
    const bool do_bias = p.bias_partial && at == 0;
    float bsum = 0.f;  // thread (channel tid & 127, groups of parity tid >> 7) of the G tile
    if (c_lo < c_hi) stage(c_lo, 0);
    __syncthreads();  // (hipcc drains vmcnt before the barrier)
    for (int c = c_lo; c < c_hi; ++c) {
        const int b = (c - c_lo) & 1;
        if (c + 1 < c_hi) stage(c + 1, b ^ 1);  // lands while this chunk is multiplied
        const char* gs = wg16_smem + b * buf_bytes;
        const char* as = gs + g_bytes;
        if (do_bias) {
            const int ch = tid & 127;
#pragma unroll
            for (int gi = tid >> 7; gi < GPC; gi += 2) {
                const char* q = gs + (gi * 4 + (ch >> 5)) * 1024 + (ch & 31) * 16;
                const bf16x8 h = *reinterpret_cast<const bf16x8*>(q), l = *reinterpret_cast<const bf16x8*>(q + 512);
#pragma unroll
                for (int e = 0; e < 8; ++e) bsum += (float)h[e] + (float)l[e];  // (hi + lo is exact in fp32)
            }
        }
#pragma unroll
        for (int s = 0; s < R / 16; ++s) {
            const int gi = 2 * s + hf;
            bf16x8 gh[2], gl[2], ah[AJ], al[AJ];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const char* q = gs + (gi * 4 + gw * 2 + i) * 1024 + li * 16;
                gh[i] = *reinterpret_cast<const bf16x8*>(q);
                gl[i] = *reinterpret_cast<const bf16x8*>(q + 512);
            }
#pragma unroll
            for (int j = 0; j < AJ; ++j) {
                const char* q = as + (gi * NBA + aw * AJ + j) * 1024 + li * 16;
                ah[j] = *reinterpret_cast<const bf16x8*>(q);
                al[j] = *reinterpret_cast<const bf16x8*>(q + 512);
            }
            // the engine's order: the two cross terms, then hi hi
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < AJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gh[i], al[j], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < AJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gl[i], ah[j], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < AJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gh[i], ah[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();  // the next chunk landed, everyone is done with this one
    }
    if (do_bias) {
        float* red = reinterpret_cast<float*>(wg16_smem);
        red[tid] = bsum;  // [parity][128 channels]
        __syncthreads();
        const int ch = gt * 128 + tid;
        if (tid < 128 && ch < p.n_gblk * 32) p.bias_partial[(size_t)split * p.n_gblk * 32 + ch] = red[tid] + red[128 + tid];
    }
    const int gpad = p.n_gblk * 32, apad = p.n_ablk * 32;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < AJ; ++j) {
            const int gblk = gt * 4 + gw * 2 + i, ablk = at * NBA + aw * AJ + j;
            if (gblk >= p.n_gblk || ablk >= p.n_ablk) continue;
            float* dst = p.partial + ((size_t)split * gpad + gblk * 32) * apad + ablk * 32 + li;
#pragma unroll
            for (int r = 0; r < 16; ++r) dst[(size_t)((r & 3) + 8 * (r >> 2) + 4 * hf) * apad] = acc[i][j][r];
        }
}

template <int AJ, int R>
constexpr int wgrad_bf16x3_lds() {
    return 2 * (R / 8) * (4 + 2 * AJ) * 1024;
}
#endif

}  // namespace hificar
