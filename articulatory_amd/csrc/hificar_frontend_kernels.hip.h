// The low-rate front end of the inversion models (egs/ema/voc1/local/predict_ema.py:83-101): features as the speech model or the MFCC
// extraction delivers them -> the model's input rows, without a stretched or normalised copy of the input in between.
//   frontend_stats_kernel    zscore (predict_ema.py:32-35, scipy.stats.zscore(axis=None)): per utterance, mean and 1 / std (population)
//                            over the C x l elements of its valid frames, two passes in double
//   frontend_rows_kernel     x (B, C, Tl) -> channels-last rows [b f Tl + t][Cp] at f times the rate, by torch's rule for
//                            F.interpolate(size=f l, mode='linear', align_corners=False) (predict_ema.py:86-90), every sequence clamped at
//                            its own first and last frame; the statistics applied on the way.  SPLIT: the rows as the bf16x3 GEMMs' split
//                            rows (xfmr_rows_split_kernel's format and expression)
//   frontend_lengths_kernel  the low-rate frame counts times f, for every kernel behind the front end
//   bigru_interp_gates_kernel  the same rule on rows [b Tl + i][N] -> [b f Tl + t][N]: the BiGRU's layer-1 pre-gates, projected at the low
//                            rate (interp(X) W + b = interp(X W + b): the two weights of a frame sum to one)
//   bigru_interp_gates_adj_kernel  its adjoint, rows [b f Tl + t][N] -> [b Tl + i][N]: the gradient of the pre-gates back at the low rate, in
//                            front of layer 1's dW_ih, db_ih and dX when the BiGRU trains on low-rate inputs (hificar_bigru_backward_lowrate)
// Fixed summation order, no atomics: an utterance's result does not depend on what it is batched with.
#pragma once
#include <hip/hip_runtime.h>

#include "hificar_bigru_train_kernels.hip.h"  // (the tape header and frame counts the adjoint kernel goes by)

namespace hificar {

constexpr int kFrontMaxFactor = 16;  // HIFICAR_LOWRATE_MAX_FACTOR

// Output frame t of a sequence of l >= 1 low-rate frames at factor f: src = max(0, (t + 0.5) / f - 0.5) = max(0, (2 t + 1 - f) / (2 f)),
// i0 = floor(src), i1 = min(i0 + 1, l - 1), lam = src - i0 — in integers, so lam is the correctly rounded fraction at any t.  t < f l.
__device__ __forceinline__ void front_source(int t, int f, int l, int& i0, int& i1, float& lam) {
    const int num = 2 * t + 1 - f;
    if (num <= 0) {
        i0 = 0;
        lam = 0.f;
    } else {
        i0 = num / (2 * f);
        lam = (float)(num - i0 * 2 * f) / (float)(2 * f);
    }
    i0 = min(i0, l - 1);
    i1 = min(i0 + 1, l - 1);
    if (i1 == i0) lam = 0.f;  // clamped at the last frame: the frame itself, bit for bit (l = 1 repeats its frame)
}

// (lam = 0: the frame itself, bit for bit — f = 1 is the identity whatever the neighbour holds)
__device__ __forceinline__ float front_mix(float a, float b, float lam) { return lam == 0.f ? a : (1.f - lam) * a + lam * b; }

// One workgroup per utterance: stats[b] = (mean, 1 / std) as doubles over x[b, :, :l] (l = the utterance's own frame count; padded frames are
// not read).  Pass 1 sums the elements, pass 2 the squares of their distances from the mean; a thread sums its elements in index order, a
// wave's lanes are summed by a butterfly, the four waves in wave order.  l = 0: (0, 0), which nothing applies.
__global__ __launch_bounds__(256) void frontend_stats_kernel(const float* __restrict__ x, const int* __restrict__ lengths, double* __restrict__ stats, int C,
                                                             int Tl) {
    __shared__ double part[4];
    __shared__ double total;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int l = lengths ? min(max(lengths[b], 0), Tl) : Tl;
    const long long n = (long long)C * l;
    const float* const xb = x + (size_t)b * C * Tl;
    double mean = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
        double acc = 0.0;
        for (long long e = tid; e < n; e += 256) {
            const int c = (int)(e / l), t = (int)(e - (long long)c * l);
            const double v = (double)xb[(size_t)c * Tl + t];
            acc += pass == 0 ? v : (v - mean) * (v - mean);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
        if ((tid & 63) == 0) part[tid >> 6] = acc;
        __syncthreads();
        if (tid == 0) total = ((part[0] + part[1]) + part[2]) + part[3];
        __syncthreads();
        const double s = total;
        __syncthreads();  // (part and total are written again by the second pass)
        if (pass == 0) mean = n > 0 ? s / (double)n : 0.0;
        else if (tid == 0) {
            stats[2 * b] = mean;
            stats[2 * b + 1] = n > 0 ? 1.0 / sqrt(s / (double)n) : 0.0;  // std = 0: 1 / 0, and (x - mean) * inf = NaN as IEEE's 0 / 0 is
        }
    }
}

// The frame counts the kernels behind the front end go by: out[b] = f * clamp(lengths[b], 0, Tl)
__global__ __launch_bounds__(256) void frontend_lengths_kernel(const int* __restrict__ lengths, int* __restrict__ out, int B, int Tl, int f) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B) out[b] = f * min(max(lengths[b], 0), Tl);
}

constexpr int kFrontSrcMax = 33;  // at most ceil(31 / f) + 2 source frames under 32 output frames (i0 advances by at most ceil(31 / f), + i1), f >= 1

// grid (ceil(f Tl / 32), Cp / 32, B).  The tile is loaded at the low rate — source frames s0 .. s0 + ceil(31 / f) + 1, each index clamped into the
// sequence's own [0, l - 1], so nothing outside x[b, :, :l] is addressed whatever `lengths` holds — and the 32 output frames are formed
// from it as they are written.  Columns C .. Cp - 1 and frames at or past f l are zeros written without reading.  stats (null: none):
// (x - mean) * (1 / std) in double, rounded once, on the way into the tile.
// SPLIT: rows [b T + t][hi: Cp bf16 | lo: Cp bf16], one 16-byte store per thread; rows32 (may be null) the fp32 rows beside them.
template <bool SPLIT>
__global__ __launch_bounds__(256) void frontend_rows_kernel(const float* __restrict__ x, float* __restrict__ rows32, char* __restrict__ rows16,
                                                            const int* __restrict__ lengths, const double* __restrict__ stats, int C, int Cp, int Tl,
                                                            int f) {
    __shared__ float tile[32][kFrontSrcMax + 2];  // (an odd stride: the writers walk the channels)
    const int b = blockIdx.z, c0 = blockIdx.y * 32, t0 = blockIdx.x * 32;
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    const int T = f * Tl;
    const int l = lengths ? min(max(lengths[b], 0), Tl) : Tl;
    const int len = f * l;
    const int ns = (31 + f - 1) / f + 2;
    int s0 = 0;
    if (t0 < len) {  // (so l >= 1)
        int i1;
        float lam;
        front_source(t0, f, l, s0, i1, lam);
        double mu = 0.0, rs = 1.0;
        if (stats) {
            mu = stats[2 * b];
            rs = stats[2 * b + 1];
        }
        for (int k = tid; k < 32 * ns; k += 256) {
            const int r = k / ns, j = k - r * ns;
            const int c = c0 + r, i = min(s0 + j, l - 1);
            float v = 0.f;
            if (c < C) {
                v = x[((size_t)b * C + c) * Tl + i];
                if (stats) v = (float)(((double)v - mu) * rs);
            }
            tile[r][j] = v;
        }
    }
    __syncthreads();
    const size_t base = (size_t)b * T;
    if (!SPLIT || rows32)
        for (int r = ty; r < 32; r += 8) {
            const int t = t0 + r, c = c0 + tx;
            if (t >= T || c >= Cp) continue;
            float v = 0.f;
            if (t < len) {
                int i0, i1;
                float lam;
                front_source(t, f, l, i0, i1, lam);
                v = front_mix(tile[tx][i0 - s0], tile[tx][i1 - s0], lam);
            }
            rows32[(base + t) * Cp + c] = v;
        }
    if constexpr (SPLIT) {
        const int r = tid >> 3, half = (tid >> 2) & 1, c8 = (tid & 3) * 8;
        const int t = t0 + r;
        if (t >= T || c0 + c8 >= Cp) return;  // (32 | Cp)
        int i0 = 0, i1 = 0;
        float lam = 0.f;
        if (t < len) front_source(t, f, l, i0, i1, lam);
        bf16x8 v;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float a = t < len ? front_mix(tile[c8 + e][i0 - s0], tile[c8 + e][i1 - s0], lam) : 0.f;
            const __bf16 hi = (__bf16)a;
            v[e] = half ? (__bf16)(a - (float)hi) : hi;
        }
        *reinterpret_cast<bf16x8*>(rows16 + (base + t) * (size_t)Cp * 4 + (half ? 2 * Cp : 0) + 2 * (c0 + c8)) = v;
    }
}

// g [b Tl + i][N] -> y [b f Tl + t][N], N a multiple of 4: one thread per float4 of an output row, 16-byte loads and stores; grid
// (ceil(f Tl N / 4 / 256), 1, B).  Rows at or past f lengths[b] are left as they are: bigru_rec_kernel reads a sequence's own frames
// only, and the head writes zeros there.
__global__ __launch_bounds__(256) void bigru_interp_gates_kernel(const float* __restrict__ g, float* __restrict__ y, const int* __restrict__ lengths, int N4,
                                                                 int Tl, int f) {
    const int b = blockIdx.z;
    const int l = lengths ? min(max(lengths[b], 0), Tl) : Tl;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const int t = (int)(e / N4), k = (int)(e - (long long)t * N4);
    if (t >= f * l) return;
    int i0, i1;
    float lam;
    front_source(t, f, l, i0, i1, lam);
    const float4 u = reinterpret_cast<const float4*>(g)[((size_t)b * Tl + i0) * N4 + k];
    const float4 v = reinterpret_cast<const float4*>(g)[((size_t)b * Tl + i1) * N4 + k];
    reinterpret_cast<float4*>(y)[((size_t)b * f * Tl + t) * N4 + k] =
        make_float4(front_mix(u.x, v.x, lam), front_mix(u.y, v.y, lam), front_mix(u.z, v.z, lam), front_mix(u.w, v.w, lam));
}

// The first output frame whose i0 (before the clamp at l - 1) is j: front_source's num = 2 t + 1 - f reaches 2 f j at
// t = f j + ceil((f - 1) / 2) = f j + f / 2; frame 0 also takes every t with 2 t + 1 <= f.
__host__ __device__ __forceinline__ int front_first_frame(int j, int f) { return j <= 0 ? 0 : f * j + f / 2; }

// The adjoint of bigru_interp_gates_kernel, for training (hificar_bigru_backward_lowrate): d [b f Tl + t][N] -> dl [b Tl + i][N],
// dl[i] = sum over t of A[t][i] d[t] with A the interpolation matrix of front_source.  A gather: low-rate frame i receives (1 - lam_t) d[t]
// from the frames whose i0 is i and lam_t d[t] from those whose i1 is i (i1 != i0: lam_t != 0), and by front_source these are ONE
// contiguous run of t: from the first frame whose i0 is i - 1 (i = 0: from 0) up to the first frame whose i0 is i + 1 (i = l - 1: up to f l,
// every frame clamped at the last one).  One thread per float4 of a low-rate row sums its run in ascending t: no atomics, one order, so an
// utterance's gradient has the same bits in any batch.  l = the sequence's own low-rate frame count, (the tape's model-rate count) / f; rows
// i >= l are written as zeros, and d is not read at or past f l.  16-byte loads and stores; grid (ceil(Tl N / 4 / 256), 1, B).
__global__ __launch_bounds__(256) void bigru_interp_gates_adj_kernel(const float* __restrict__ d, float* __restrict__ dl, const BigruTapeHeader* hdr,
                                                                     const int* __restrict__ tape_lens, int N4, int Tl, int f) {
    const int b = blockIdx.z;
    const int l = bigru_len(bigru_tape_lens(hdr, tape_lens), b, f * Tl) / f;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const int i = (int)(e / N4), k = (int)(e - (long long)i * N4);
    if (i >= Tl) return;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < l) {
        const int t_end = i == l - 1 ? f * l : front_first_frame(i + 1, f);
        const float4* const src = reinterpret_cast<const float4*>(d) + (size_t)b * f * Tl * N4 + k;
        for (int t = front_first_frame(i - 1, f); t < t_end; ++t) {
            int i0, i1;
            float lam;
            front_source(t, f, l, i0, i1, lam);
            const float w = i0 == i ? 1.f - lam : lam;  // (i0 = i - 1 and i1 = i otherwise; lam = 0 there: the frame gives nothing)
            if (w == 0.f) continue;
            const float4 v = src[(size_t)t * N4];
            acc.x += w * v.x;
            acc.y += w * v.y;
            acc.z += w * v.z;
            acc.w += w * v.w;
        }
    }
    reinterpret_cast<float4*>(dl)[((size_t)b * Tl + i) * N4 + k] = acc;
}

}  // namespace hificar
