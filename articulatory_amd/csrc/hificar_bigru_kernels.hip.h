// Kernels of the BiGRU inversion model (articulatory/models/pytorch_models.py:22-72): the recurrent sweep of one bidirectional GRU layer,
// the (B, C, T) -> channels-last gather in front of the first input projection, and the fc2 (+ tanh) head.  The input projections and fc1
// run on the conv engine (one-tap GEMMs, hificar_bigru.hip.inc).
#pragma once
#include <hip/hip_runtime.h>

namespace hificar {

typedef float bigru_f2 __attribute__((ext_vector_type(2)));

// How one direction's W_hh (3H x H) is spread over a workgroup of 2H threads.  Thread tid = 2 i + q owns the three gate rows (r, z, n) of
// hidden unit i over the k range [q H/2, (q + 1) H/2): 3 H/2 weights, of which the first KR columns per row stay in registers for the whole
// sweep, the next KL in an LDS slab, and the last KG are streamed from L2 every step.  At H = 256 with one sequence per workgroup that is
// 336 KiB in registers, 144 KiB in LDS and 288 KiB streamed per step; H <= 128 is fully resident.  The packed layout does not depend on
// the split.
template <int H, int NS>
struct BigruSplit {
    static constexpr int NT = 2 * H;
    static constexpr int KH = H / 2;
    static constexpr int KRMAX = NS == 1 ? (KH <= 64 ? 64 : 56) : 40;  // what 256 registers leave beside the working set: no scratch
    static constexpr int KR = KH < KRMAX ? KH : KRMAX;
    static constexpr int KL = (KH - KR) < 24 ? (KH - KR) : 24;
    static constexpr int KG = KH - KR - KL;
    static constexpr int CH = KH / 4, CR = KR / 4, CL = KL / 4, CG = KG / 4;  // in float4 columns
    static_assert(H % 64 == 0 && H >= 64 && H <= 256, "hidden sizes: multiples of 64 up to 256");
    static constexpr size_t lds_bytes = (size_t)3 * CL * NT * 16 + (size_t)2 * NS * H * 4;
};

struct BigruRecParams {
    const float* g;       // pre-gates [B * T][6H]: W_ih x + b_ih, forward r | z | n, then reverse r | z | n
    const float4* w;      // packed W_hh: [dir][gate * CH + column][2H threads] float4 (hificar_bigru.hip.inc: pack_whh)
    const float* bhh;     // [dir][3H]
    const int* lengths;   // B frame counts on the device, or null: all T
    float* y;             // [B * T][2H]: forward | reverse hidden states; rows at or past a sequence's length are not written
    int B, T;
    float* tape = nullptr;  // TAPE instantiations (training): [B * T][2][4H], r | z | n | W_hn h + b_hn of every (frame, direction)
};

__device__ __forceinline__ void bigru_fma4(bigru_f2& acc, const float4& w, const float4& h) {
    acc = __builtin_elementwise_fma(bigru_f2{w.x, w.y}, bigru_f2{h.x, h.y}, acc);
    acc = __builtin_elementwise_fma(bigru_f2{w.z, w.w}, bigru_f2{h.z, h.w}, acc);
}

__device__ __forceinline__ float bigru_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// One workgroup sweeps NS sequences of one direction from their first step to their last; nothing is shared between workgroups.  PyTorch's
// GRU cell (gate order r, z, n; h0 = 0):  r = s(gx_r + W_hr h + b_hr), z = s(gx_z + W_hz h + b_hz), n = tanh(gx_n + r (W_hn h + b_hn)),
// h' = (1 - z) n + z h.  The reverse direction starts at each sequence's own last frame.  A sequence's arithmetic does not depend on NS or on
// its neighbours in the tile: every dot product is summed in the same order.  TAPE: the same sweep, and what the backward sweep reads per
// (direction, frame) is kept (hificar_bigru_train_kernels.hip.h); the arithmetic of h is the same statement for statement.
template <int H, int NS, bool TAPE = false>
__global__ __launch_bounds__(2 * H) void bigru_rec_kernel(const BigruRecParams p) {
    using S = BigruSplit<H, NS>;
    constexpr int NT = S::NT, CH = S::CH, CR = S::CR, CL = S::CL, CG = S::CG;
    extern __shared__ float4 bigru_smem[];
    float4* const wl = bigru_smem;                                          // [3 * CL][NT]
    float* const hbuf = reinterpret_cast<float*>(bigru_smem + 3 * CL * NT);  // [2][NS][H]
    const int tid = threadIdx.x, q = tid & 1, i = tid >> 1;
    const int dir = blockIdx.y, s0 = blockIdx.x * NS;
    const float4* const wd = p.w + (size_t)dir * 3 * CH * NT;

    float4 wr[3][CR > 0 ? CR : 1];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int c = 0; c < CR; ++c) wr[g][c] = wd[(size_t)(g * CH + c) * NT + tid];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int c = 0; c < CL; ++c) wl[(g * CL + c) * NT + tid] = wd[(size_t)(g * CH + CR + c) * NT + tid];
    float bh[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) bh[g] = p.bhh[(size_t)dir * 3 * H + g * H + i];

    int len[NS], nmax = 0;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int b = s0 + s;
        len[s] = b < p.B ? (p.lengths ? min(max(p.lengths[b], 0), p.T) : p.T) : 0;
        nmax = max(nmax, len[s]);
    }
    for (int k = tid; k < 2 * NS * H; k += NT) hbuf[k] = 0.f;
    __syncthreads();

    const size_t gstride = (size_t)6 * H;
    auto frame = [&](int s, int n) { return dir == 0 ? n : len[s] - 1 - n; };
    auto load_gx = [&](int s, int n, float (&gx)[3]) {
        if (n < len[s]) {
            const float* row = p.g + ((size_t)(s0 + s) * p.T + frame(s, n)) * gstride + (size_t)dir * 3 * H + i;
#pragma unroll
            for (int g = 0; g < 3; ++g) gx[g] = row[g * H];
        } else {
#pragma unroll
            for (int g = 0; g < 3; ++g) gx[g] = 0.f;
        }
    };

    float hown[NS], gx[NS][3];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        hown[s] = 0.f;
        load_gx(s, 0, gx[s]);
    }

    for (int n = 0; n < nmax; ++n) {
        const int cur = n & 1;
        float gnext[NS][3];
#pragma unroll
        for (int s = 0; s < NS; ++s) load_gx(s, n + 1, gnext[s]);

        bigru_f2 acc[NS][3];
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int g = 0; g < 3; ++g) acc[s][g] = bigru_f2{0.f, 0.f};
        const float4* const h4 = reinterpret_cast<const float4*>(hbuf + cur * NS * H) + q * CH;
#pragma unroll
        for (int c = 0; c < CR; ++c)
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const float4 hv = h4[s * (H / 4) + c];
#pragma unroll
                for (int g = 0; g < 3; ++g) bigru_fma4(acc[s][g], wr[g][c], hv);
            }
#pragma unroll
        for (int c = 0; c < CL; ++c) {
            float4 w[3];
#pragma unroll
            for (int g = 0; g < 3; ++g) w[g] = wl[(g * CL + c) * NT + tid];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const float4 hv = h4[s * (H / 4) + CR + c];
#pragma unroll
                for (int g = 0; g < 3; ++g) bigru_fma4(acc[s][g], w[g], hv);
            }
        }
#pragma unroll 4
        for (int c = 0; c < CG; ++c) {
            float4 w[3];
#pragma unroll
            for (int g = 0; g < 3; ++g) w[g] = wd[(size_t)(g * CH + CR + CL + c) * NT + tid];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const float4 hv = h4[s * (H / 4) + CR + CL + c];
#pragma unroll
                for (int g = 0; g < 3; ++g) bigru_fma4(acc[s][g], w[g], hv);
            }
        }

        float* const hnext = hbuf + (cur ^ 1) * NS * H;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            float d[3];
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                const float part = acc[s][g].x + acc[s][g].y;
                d[g] = part + __shfl_xor(part, 1) + bh[g];  // the two halves of the row (commutative: both lanes get the same bits)
            }
            if (n < len[s]) {
                const float r = bigru_sigmoid(gx[s][0] + d[0]);
                const float z = bigru_sigmoid(gx[s][1] + d[1]);
                const float c = tanhf(gx[s][2] + r * d[2]);
                hown[s] = (1.f - z) * c + z * hown[s];
                if (q == 0) p.y[((size_t)(s0 + s) * p.T + frame(s, n)) * (2 * H) + dir * H + i] = hown[s];
                if constexpr (TAPE) {
                    if (q == 0) {
                        float* tp = p.tape + (((size_t)(s0 + s) * p.T + frame(s, n)) * 2 + dir) * (4 * H) + i;
                        tp[0] = r;
                        tp[H] = z;
                        tp[2 * H] = c;
                        tp[3 * H] = d[2];
                    }
                }
            }
            if (q == 0) hnext[s * H + i] = hown[s];
#pragma unroll
            for (int g = 0; g < 3; ++g) gx[s][g] = gnext[s][g];
        }
        __syncthreads();  // step n's reads of hbuf[cur] are done and hbuf[cur ^ 1] is complete: the one barrier of a step
    }
}

// x (B, C, T) fp32 -> rows [b * T + t][Cp] (channels last, columns C .. Cp - 1 zero): the input rows of the first projection GEMM.
__global__ __launch_bounds__(256) void bigru_rows_kernel(const float* __restrict__ x, float* __restrict__ rows, int C, int Cp, int T) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z, c0 = blockIdx.y * 32, t0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const int c = c0 + r, t = t0 + tx;
        tile[r][tx] = (c < C && t < T) ? x[((size_t)b * C + c) * T + t] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int t = t0 + r, c = c0 + tx;
        if (t < T && c < Cp) rows[((size_t)b * T + t) * Cp + c] = tile[tx][r];
    }
}

constexpr int kBigruFc1 = 128;     // Linear(2H, 128) + BatchNorm1d(128) (pytorch_models.py:32-33)
constexpr int kBigruMaxOut = 32;   // fc2's rows held in LDS by the head kernel

struct BigruHeadParams {
    const float* f;      // [B * T][128]: fc1 with the batch norm folded in
    const float* w2;     // (O, 128)
    const float* b2;     // (O)
    const int* lengths;  // device, or null
    float* out;          // (B, O, T); frames at or past a sequence's length are written as zeros
    int B, T, O, use_tanh;
};

// fc2 (+ tanh) over a tile of 64 frames of one sequence, written in the reference's (B, C, T) layout (pytorch_models.py:71).
__global__ __launch_bounds__(256) void bigru_head_kernel(const BigruHeadParams p) {
    __shared__ float tile[64][kBigruFc1 + 1];
    __shared__ float w[kBigruMaxOut * kBigruFc1];
    const int b = blockIdx.y, t0 = blockIdx.x * 64, tid = threadIdx.x;
    for (int k = tid; k < p.O * kBigruFc1; k += 256) w[k] = p.w2[k];
    for (int k = tid; k < 64 * kBigruFc1; k += 256) {
        const int r = k / kBigruFc1, c = k % kBigruFc1;
        tile[r][c] = t0 + r < p.T ? p.f[((size_t)b * p.T + t0 + r) * kBigruFc1 + c] : 0.f;
    }
    __syncthreads();
    const int tl = tid & 63, t = t0 + tl;
    const int len = p.lengths ? min(max(p.lengths[b], 0), p.T) : p.T;
    if (t >= p.T) return;
    for (int o = tid >> 6; o < p.O; o += 4) {
        float acc = 0.f;
#pragma unroll 8
        for (int k = 0; k < kBigruFc1; ++k) acc = fmaf(tile[tl][k], w[o * kBigruFc1 + k], acc);
        acc += p.b2[o];
        if (p.use_tanh) acc = tanhf(acc);
        p.out[((size_t)b * p.O + o) * p.T + t] = t < len ? acc : 0.f;
    }
}

}  // namespace hificar
