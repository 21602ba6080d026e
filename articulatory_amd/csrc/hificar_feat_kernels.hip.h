// Speech features on the device (hificar_feat.hip.inc): MFCC as egs/ema/voc1/local/predict_ema.py:32-33 takes it from librosa 0.8.1
// (melspectrogram(power=2) -> power_to_db -> orthonormal DCT-II) and the log-mel filterbank of articulatory/bin/preprocess.py:58-82, for a
// ragged batch of waveforms.  The DFT is one GEMM on the exact-fp32 conv kernels (window folded into the matrix); these are the passes
// around it.
//   feat_frame_kernel       wav (B, Lmax) -> rows A[(b, t)][n] = y_b[reflect(t hop + n - N / 2)], every utterance reflected at its own two
//                           ends; rows t >= T_b are zeros written without reading
//   feat_mel_kernel         S [M][re | im] -> V [M][num_mels]: a thread owns a (frame, band) and walks the band's triangle in ascending bin
//                           order.  MFCC: 10 log10(max(amin, sum w (re^2 + im^2))); log-mel: sum w sqrt(re^2 + im^2)
//   feat_db_max_kernel      MFCC: per utterance the maximum of V over its own T_b x num_mels elements (power_to_db's top_db reference)
//   feat_mfcc_out_kernel    max(V, max_b - top_db) -> DCT against a host-built basis -> out (B, n_mfcc, Tmax), zeros from T_b on
//   feat_logmel_out_kernel  log_b(max(eps, V)) -> out (B, num_mels, Tmax), zeros from T_b on
// Fixed summation order, no atomics: an utterance's result does not depend on what it is batched with.  Samples at or past an utterance's
// length are never read.
#pragma once
#include <hip/hip_runtime.h>

#include "hificar_disc_kernels.hip.h"  // reflect_index

namespace hificar {

// frames of an utterance of l samples: 1 + l / hop (librosa.stft(center=True)); an utterance too short to reflect (l <= N / 2, which the host
// refuses wherever it sees the lengths) has none, so that nothing outside [0, l) is ever addressed
__device__ __forceinline__ int feat_frames(const int* __restrict__ lengths, int b, int Lmax, int N, int hop, int& l) {
    l = lengths ? min(max(lengths[b], 0), Lmax) : Lmax;
    return l > N / 2 ? 1 + l / hop : 0;
}

struct FeatFrameParams {
    const float* wav;    // (B, Lmax)
    const int* lengths;  // [B] or null
    float* A;            // [B * Tmax][N]
    long long total4;    // B * Tmax * N / 4
    int Lmax, N, hop, Tmax;
};

__global__ __launch_bounds__(256) void feat_frame_kernel(const FeatFrameParams p) {
    const int n4 = p.N >> 2;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < p.total4; i += (long long)gridDim.x * 256) {
        const int m = (int)(i / n4), n = (int)(i - (long long)m * n4) * 4;
        const int b = m / p.Tmax, t = m - b * p.Tmax;
        int l;
        const int Tb = feat_frames(p.lengths, b, p.Lmax, p.N, p.hop, l);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (t < Tb) {  // (l > N / 2: one reflection lands inside [0, l))
            const float* const y = p.wav + (size_t)b * p.Lmax;
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = y[reflect_index(t * p.hop + n + u - p.N / 2, l)];
        }
        reinterpret_cast<f32x4*>(p.A)[i] = v;  // (16-byte store: N is a multiple of 32, A 256-byte aligned)
    }
}

struct FeatMelParams {
    const float* S;      // [M][2 * nfp]: re at [0, nfp), im at [nfp, 2 nfp)
    const int* band;     // [nm][2]: first bin, number of bins of the band's triangle
    const float* w;      // [nm][wmax]: the filterbank's weights over those bins
    float* V;            // [M][nm]
    long long total;     // M * nm
    int nm, nfp, wmax;
    float amin;          // MFCC: the floor under the log
};

template <bool MFCC>
__global__ __launch_bounds__(256) void feat_mel_kernel(const FeatMelParams p) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < p.total; i += (long long)gridDim.x * 256) {
        const int m = (int)(i / p.nm), k = (int)(i - (long long)m * p.nm);
        const int f0 = p.band[2 * k], nb = p.band[2 * k + 1];
        const float* const re = p.S + (size_t)m * 2 * p.nfp + f0;
        const float* const im = re + p.nfp;
        const float* const w = p.w + (size_t)k * p.wmax;
        float acc = 0.f;
        for (int j = 0; j < nb; ++j) {
            const float pw = re[j] * re[j] + im[j] * im[j];
            acc = fmaf(w[j], MFCC ? pw : sqrtf(pw), acc);
        }
        p.V[i] = MFCC ? 10.f * log10f(fmaxf(p.amin, acc)) : acc;
    }
}

// One workgroup per utterance: maxv[b] = the maximum over V[b Tmax .. b Tmax + T_b) x num_mels, which is one contiguous run.  A thread takes
// the maximum of its elements in index order, a wave's lanes meet in a butterfly, the four waves in wave order.  T_b = 0: -inf, which nothing reads.
__global__ __launch_bounds__(256) void feat_db_max_kernel(const float* __restrict__ V, const int* __restrict__ lengths, float* __restrict__ maxv, int nm,
                                                          int Lmax, int N, int hop, int Tmax) {
    __shared__ float part[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    int l;
    const int Tb = feat_frames(lengths, b, Lmax, N, hop, l);
    const long long n = (long long)Tb * nm;
    const float* const v = V + (size_t)b * Tmax * nm;
    float acc = -INFINITY;
    for (long long e = tid; e < n; e += 256) acc = fmaxf(acc, v[e]);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc = fmaxf(acc, __shfl_xor(acc, m));
    if ((tid & 63) == 0) part[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) maxv[b] = fmaxf(fmaxf(fmaxf(part[0], part[1]), part[2]), part[3]);
}

constexpr int kFeatMaxMels = 128;  // HIFICAR_FEAT_MAX_MELS

struct FeatOutParams {
    const float* V;      // [M][nm]
    const int* lengths;  // [B] or null
    const float* maxv;   // MFCC: [B]
    const float* basis;  // MFCC: [nc][nm] orthonormal DCT-II rows
    float* out;          // (B, nc, Tmax)
    int* frames_out;     // [B] or null
    int nm, nc, Lmax, N, hop, Tmax;
    float top_db;        // MFCC: < 0 = no clamp
    float eps;           // log-mel: the floor under the log
    int log_base;        // log-mel: 0 natural, 2, 10
};

// Both output kernels: grid (ceil(Tmax / 32), B), 32 frames per workgroup.  The 32 x nm values are one contiguous run of V: they are loaded
// with consecutive lanes on consecutive addresses into a tile whose rows are one float longer than nm is rounded up to an even number (an
// odd stride), so that the second phase — lane = frame, the fastest index of the (B, C, Tmax) output — reads the tile down a column without
// bank conflicts and stores 32 consecutive floats per channel.
__device__ __forceinline__ int feat_tile_stride(int nm) { return nm | 1; }

__global__ __launch_bounds__(256) void feat_mfcc_out_kernel(const FeatOutParams p) {
    __shared__ float tile[32 * (kFeatMaxMels + 1)];
    const int b = blockIdx.y, t0 = blockIdx.x * 32, tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    const int ld = feat_tile_stride(p.nm);
    int l;
    const int Tb = feat_frames(p.lengths, b, p.Lmax, p.N, p.hop, l);
    if (blockIdx.x == 0 && tid == 0 && p.frames_out) p.frames_out[b] = Tb;
    const int nt = min(32, Tb - t0);  // valid frames of this tile (<= 0: none)
    if (nt > 0) {
        const float floor_db = p.top_db >= 0.f ? p.maxv[b] - p.top_db : -INFINITY;
        const float* const v = p.V + ((size_t)b * p.Tmax + t0) * p.nm;
        for (int e = tid; e < nt * p.nm; e += 256) {
            const int r = e / p.nm, k = e - r * p.nm;
            tile[r * ld + k] = fmaxf(v[e], floor_db);
        }
    }
    __syncthreads();
    const int t = t0 + tx;
    if (t >= p.Tmax) return;
    for (int c = ty; c < p.nc; c += 8) {
        float acc = 0.f;
        if (tx < nt) {
            const float* const bc = p.basis + (size_t)c * p.nm;
            for (int k = 0; k < p.nm; ++k) acc = fmaf(bc[k], tile[tx * ld + k], acc);
        }
        p.out[((size_t)b * p.nc + c) * p.Tmax + t] = acc;
    }
}

__global__ __launch_bounds__(256) void feat_logmel_out_kernel(const FeatOutParams p) {
    __shared__ float tile[32 * (kFeatMaxMels + 1)];
    const int b = blockIdx.y, t0 = blockIdx.x * 32, tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    const int ld = feat_tile_stride(p.nm);
    int l;
    const int Tb = feat_frames(p.lengths, b, p.Lmax, p.N, p.hop, l);
    if (blockIdx.x == 0 && tid == 0 && p.frames_out) p.frames_out[b] = Tb;
    const int nt = min(32, Tb - t0);
    if (nt > 0) {
        const float* const v = p.V + ((size_t)b * p.Tmax + t0) * p.nm;
        for (int e = tid; e < nt * p.nm; e += 256) {
            const int r = e / p.nm, k = e - r * p.nm;
            const float x = fmaxf(p.eps, v[e]);
            tile[r * ld + k] = p.log_base == 10 ? log10f(x) : p.log_base == 2 ? log2f(x) : logf(x);
        }
    }
    __syncthreads();
    const int t = t0 + tx;
    if (t >= p.Tmax) return;
    for (int c = ty; c < p.nm; c += 8) p.out[((size_t)b * p.nm + c) * p.Tmax + t] = tx < nt ? tile[tx * ld + c] : 0.f;
}

}  // namespace hificar
