// Training kernels of the BiGRU inversion model (the reference's train() mode: articulatory/models/pytorch_models.py:45-72 under autograd):
// counter-based dropout, BatchNorm1d on batch statistics, the fc2 head forwards and backwards, and the backward recurrent sweep.  The
// GEMMs (input projections, fc1, their data and weight gradients) run on the conv engine and the weight-gradient kernels
// (hificar_bigru_train.hip.inc).  Exact fp32; every reduction is summed in a fixed order (no atomics).
// Ragged batches (hificar_bigru_forward_train_ragged): the tape keeps the frame counts; every kernel below skips the frames at or past a
// sequence's count and writes zeros there, so that the GEMMs, which run over all B T rows, add nothing for them.  A dense tape
// (ragged = 0) takes the same statements with every count = T.
#pragma once
#include "hificar_bigru_kernels.hip.h"

namespace hificar {

// ------------------------------------------------------------------------------------------------
// Dropout: keep = u(seed, offset, site, element) >= p, kept values scaled by 1 / (1 - p).  The numpy restatement is
// articulatory_amd.utils.synth.bigru_dropout_mask; masks are regenerated wherever they are needed, never stored.
// ------------------------------------------------------------------------------------------------
struct BigruTapeHeader {  // the first 256 bytes of a tape: what the backward pass must know about the forward call that filled it
    unsigned long long seed, offset;
    float p;
    int B, T;
    int M;       // valid frames: the sum of the frame counts (dense: B T), what the batch statistics divide by
    int ragged;  // the tape's frame counts hold (hificar_bigru_forward_train_ragged); 0: every sequence is T frames long
    int factor, Tl, zscore;  // hificar_bigru_forward_train_lowrate: T = factor Tl, the tape's input rows are the Tl low-rate ones (z-scored); else 1, T, 0
};

// the frame counts a kernel goes by: `lens` is the tape's copy, honoured only by a ragged tape
__device__ __forceinline__ const int* bigru_tape_lens(const BigruTapeHeader* hdr, const int* lens) { return hdr->ragged ? lens : nullptr; }
__device__ __forceinline__ int bigru_len(const int* lens, int b, int T) { return lens ? min(max(lens[b], 0), T) : T; }
// row r = b T + t of a [B T] buffer is a frame of its sequence (not padding)
__device__ __forceinline__ bool bigru_row_valid(const int* lens, int r, int T) {
    if (!lens) return true;
    const int b = r / T;
    return r - b * T < min(max(lens[b], 0), T);
}
// fn(r) for the valid rows among r0, r0 + 32, ... < rows, in that order.  Dense (lens null): the plain loop.  Ragged: one division at the
// start and a frame count read per sequence entered.
template <typename F>
__device__ __forceinline__ void bigru_for_valid_rows(const int* lens, int r0, int rows, int T, F fn) {
    if (!lens) {
        for (int r = r0; r < rows; r += 32) fn(r);
        return;
    }
    int b = r0 / T, t = r0 - b * T, have = -1, len = 0;
    for (int r = r0; r < rows; r += 32) {
        if (have != b) {  // (r < rows: b < B)
            len = min(max(lens[b], 0), T);
            have = b;
        }
        if (t < len) fn(r);
        t += 32;
        while (t >= T) {
            t -= T;
            ++b;
        }
    }
}

enum { kBigruSiteGru1 = 0, kBigruSiteGru2 = 1, kBigruSiteFc1 = 2 };

__host__ __device__ __forceinline__ unsigned long long bigru_mix64(unsigned long long x) {  // splitmix64's output function
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

struct BigruDrop {
    unsigned long long key;
    float p, scale;
    __device__ __forceinline__ BigruDrop(const BigruTapeHeader* hdr, int site) {
        p = hdr->p;
        scale = p > 0.f ? 1.f / (1.f - p) : 1.f;
        key = bigru_mix64(hdr->seed ^ bigru_mix64(hdr->offset * 4ull + (unsigned long long)site));
    }
    // the factor of element e: 0 (dropped) or 1 / (1 - p); p = 0 is the identity and draws nothing
    __device__ __forceinline__ float operator()(unsigned long long e) const {
        if (!(p > 0.f)) return 1.f;
        const float u = (float)(unsigned)(bigru_mix64(key + e) >> 40) * (1.f / 16777216.f);
        return u >= p ? scale : 0.f;
    }
};

__global__ __launch_bounds__(1) void bigru_header_kernel(BigruTapeHeader* hdr, unsigned long long seed, unsigned long long offset, float p, int B, int T,
                                                         int M, int ragged, int factor, int Tl, int zscore) {
    hdr->seed = seed;
    hdr->offset = offset;
    hdr->p = p;
    hdr->B = B;
    hdr->T = T;
    hdr->M = M;
    hdr->ragged = ragged;
    hdr->factor = factor;
    hdr->Tl = Tl;
    hdr->zscore = zscore;
}

// rows[b T + t][0 .. width) = 0 for lens[b] <= t < T (width % 4 == 0): the frames a ragged sweep leaves unwritten, which later GEMMs read.
// grid (row blocks, B)
__global__ __launch_bounds__(256) void bigru_zero_pad_kernel(float* __restrict__ rows, int width, const int* __restrict__ lens, int T) {
    const int b = blockIdx.y, len = bigru_len(lens, b, T), w4 = width / 4;
    const long long n4 = (long long)(T - len) * w4;
    float4* const dst = reinterpret_cast<float4*>(rows + ((size_t)b * T + len) * width);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) dst[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// out[e] = in[e] * factor(site, e) over n elements (n % 4 == 0); in == out is allowed
__global__ __launch_bounds__(256) void bigru_dropout_kernel(const float* in, float* out, long long n, const BigruTapeHeader* hdr, int site) {
    const BigruDrop drop(hdr, site);
    for (long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; e < n; e += (long long)gridDim.x * 1024) {
        float4 v = *reinterpret_cast<const float4*>(in + e);
        v.x *= drop((unsigned long long)e);
        v.y *= drop((unsigned long long)e + 1);
        v.z *= drop((unsigned long long)e + 2);
        v.w *= drop((unsigned long long)e + 3);
        *reinterpret_cast<float4*>(out + e) = v;
    }
}

// ------------------------------------------------------------------------------------------------
// BatchNorm1d(128) on batch statistics over the valid rows of dropout(fc1): M = hdr->M of them among the `rows` = B T.
// ------------------------------------------------------------------------------------------------
// A workgroup owns 32 channels: thread (row lane ty, channel tx) sums rows ty, ty + 32, ..., then one thread per channel adds the 32 lanes
// in order.  red: [32][33] floats of LDS.  Padded rows are skipped in place: a valid row keeps its lane and its turn, so a batch
// without padding is summed exactly as a dense one.
__device__ __forceinline__ double bigru_bn_lane_sum(float (*red)[33], float v, int tx, int ty) {
    __syncthreads();
    red[ty][tx] = v;
    __syncthreads();
    double s = 0.0;
    for (int k = 0; k < 32; ++k) s += (double)red[k][tx];
    return s;
}

// stats: [mean | biased variance | 1 / sqrt(var + eps)] x 128 on the tape; batch_stats (mean | biased variance) goes back to the caller
__global__ __launch_bounds__(1024) void bigru_bn_stats_kernel(const float* __restrict__ f1, int rows, const BigruTapeHeader* hdr,
                                                              const int* __restrict__ tape_lens, float* __restrict__ stats,
                                                              float* __restrict__ batch_stats) {
    __shared__ float red[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5, c = blockIdx.x * 32 + tx;
    const BigruDrop drop(hdr, kBigruSiteFc1);
    const int* const lens = bigru_tape_lens(hdr, tape_lens);
    const int M = hdr->M, T = hdr->T;
    float s = 0.f;
    bigru_for_valid_rows(lens, ty, rows, T, [&](int r) {
        const size_t e = (size_t)r * kBigruFc1 + c;
        s += f1[e] * drop(e);
    });
    const float mean = (float)(bigru_bn_lane_sum(red, s, tx, ty) / (double)M);
    s = 0.f;
    bigru_for_valid_rows(lens, ty, rows, T, [&](int r) {
        const size_t e = (size_t)r * kBigruFc1 + c;
        const float d = f1[e] * drop(e) - mean;
        s = fmaf(d, d, s);
    });
    const float var = (float)(bigru_bn_lane_sum(red, s, tx, ty) / (double)M);
    if (ty == 0) {
        stats[c] = mean;
        stats[kBigruFc1 + c] = var;
        stats[2 * kBigruFc1 + c] = 1.f / sqrtf(var + 1e-5f);
        batch_stats[c] = mean;
        batch_stats[kBigruFc1 + c] = var;
    }
}

struct BigruHeadTrainParams {
    const float* f1;     // [B * T][128]: raw fc1 output (before dropout)
    const float* stats;  // [3][128] of bigru_bn_stats_kernel
    const float* gamma;  // bn.weight
    const float* beta;   // bn.bias
    const float* w2;     // (O, 128)
    const float* b2;     // (O)
    const BigruTapeHeader* hdr;
    const int* lens;     // the tape's frame counts (bigru_tape_lens)
    float* out;          // forward: (B, O, T); frames at or past a sequence's count: zeros
    float* out_keep;     // forward: the tape's copy of out (tanh'), same layout
    // backward
    const float* dout;   // (B, O, T); frames at or past a sequence's count are not read
    float* dbn;          // [B * T][128]: gradient of the batch norm's output
    float* pw;           // [tiles][O * 128] partials of dW_fc2
    float* pb;           // [tiles][O] partials of db_fc2
    int B, T, O, use_tanh;
};

// the head's input tile: bn(dropout(fc1)) of 64 frames (zeros from frame `len` on), recomputed from the raw fc1 rows wherever it is needed
__device__ __forceinline__ void bigru_head_load_tile(const BigruHeadTrainParams& p, float (*tile)[kBigruFc1 + 1], int b, int t0, int len, int tid) {
    const BigruDrop drop(p.hdr, kBigruSiteFc1);
    for (int k = tid; k < 64 * kBigruFc1; k += 256) {
        const int r = k / kBigruFc1, c = k % kBigruFc1;
        float v = 0.f;
        if (t0 + r < len) {
            const size_t e = ((size_t)b * p.T + t0 + r) * kBigruFc1 + c;
            v = (p.f1[e] * drop(e) - p.stats[c]) * p.stats[2 * kBigruFc1 + c] * p.gamma[c] + p.beta[c];
        }
        tile[r][c] = v;
    }
}

// dropout -> batch norm -> fc2 (+ tanh): bigru_head_kernel on the training-mode input
__global__ __launch_bounds__(256) void bigru_head_train_kernel(const BigruHeadTrainParams p) {
    __shared__ float tile[64][kBigruFc1 + 1];
    __shared__ float w[kBigruMaxOut * kBigruFc1];
    const int b = blockIdx.y, t0 = blockIdx.x * 64, tid = threadIdx.x;
    const int len = bigru_len(bigru_tape_lens(p.hdr, p.lens), b, p.T);
    for (int k = tid; k < p.O * kBigruFc1; k += 256) w[k] = p.w2[k];
    bigru_head_load_tile(p, tile, b, t0, len, tid);
    __syncthreads();
    const int tl = tid & 63, t = t0 + tl;
    if (t >= p.T) return;
    for (int o = tid >> 6; o < p.O; o += 4) {
        float acc = 0.f;
#pragma unroll 8
        for (int k = 0; k < kBigruFc1; ++k) acc = fmaf(tile[tl][k], w[o * kBigruFc1 + k], acc);
        acc += p.b2[o];
        if (p.use_tanh) acc = tanhf(acc);
        if (t >= len) acc = 0.f;
        const size_t e = ((size_t)b * p.O + o) * p.T + t;
        p.out[e] = acc;
        p.out_keep[e] = acc;
    }
}

// dout -> tanh' -> the gradient of the batch norm's output, and this tile's share of dW_fc2 / db_fc2
__global__ __launch_bounds__(256) void bigru_head_bwd_kernel(const BigruHeadTrainParams p) {
    __shared__ float tile[64][kBigruFc1 + 1];
    __shared__ float w[kBigruMaxOut * kBigruFc1];
    __shared__ float dz[64][kBigruMaxOut + 1];
    const int b = blockIdx.y, t0 = blockIdx.x * 64, tid = threadIdx.x;
    const int len = bigru_len(bigru_tape_lens(p.hdr, p.lens), b, p.T);
    for (int k = tid; k < p.O * kBigruFc1; k += 256) w[k] = p.w2[k];
    bigru_head_load_tile(p, tile, b, t0, len, tid);
    for (int k = tid; k < 64 * p.O; k += 256) {
        const int o = k >> 6, r = k & 63;
        float v = 0.f;
        if (t0 + r < len) {  // dout of a padded frame counts as zero, whatever it holds
            const size_t e = ((size_t)b * p.O + o) * p.T + t0 + r;
            v = p.dout[e];
            if (p.use_tanh) {
                const float y = p.out_keep[e];
                v *= 1.f - y * y;
            }
        }
        dz[r][o] = v;
    }
    __syncthreads();
    {
        const int k = tid & 127;
        for (int r = tid >> 7; r < 64 && t0 + r < p.T; r += 2) {
            float acc = 0.f;
            for (int o = 0; o < p.O; ++o) acc = fmaf(dz[r][o], w[o * kBigruFc1 + k], acc);
            p.dbn[((size_t)b * p.T + t0 + r) * kBigruFc1 + k] = acc;  // (padded frames: dz = 0, so zeros)
        }
    }
    const size_t part = (size_t)b * gridDim.x + blockIdx.x;
    for (int idx = tid; idx < p.O * kBigruFc1; idx += 256) {
        const int o = idx >> 7, k = idx & 127;
        float acc = 0.f;
#pragma unroll 8
        for (int r = 0; r < 64; ++r) acc = fmaf(dz[r][o], tile[r][k], acc);  // (rows past the sequence's count: dz = 0 and tile = 0)
        p.pw[part * p.O * kBigruFc1 + idx] = acc;
    }
    if (tid < p.O) {
        float acc = 0.f;
        for (int r = 0; r < 64; ++r) acc += dz[r][tid];
        p.pb[part * p.O + tid] = acc;
    }
}

// dst[j] = sum over parts of partial[part][j], in order
__global__ __launch_bounds__(256) void bigru_colreduce_kernel(const float* __restrict__ partial, int parts, int width, float* __restrict__ dst) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= width) return;
    double s = 0.0;
    for (int i = 0; i < parts; ++i) s += (double)partial[(size_t)i * width + j];
    dst[j] = (float)s;
}

// BatchNorm backward, the two per-channel sums: dbeta = sum dy, dgamma = sum dy xhat  (xhat recomputed from the raw fc1 rows)
__global__ __launch_bounds__(1024) void bigru_bn_bwd_sums_kernel(const float* __restrict__ f1, const float* __restrict__ dbn, int rows,
                                                                 const BigruTapeHeader* hdr, const int* __restrict__ tape_lens,
                                                                 const float* __restrict__ stats, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    __shared__ float red[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5, c = blockIdx.x * 32 + tx;
    const BigruDrop drop(hdr, kBigruSiteFc1);
    const int* const lens = bigru_tape_lens(hdr, tape_lens);
    const int T = hdr->T;
    const float mean = stats[c], rstd = stats[2 * kBigruFc1 + c];
    float sb = 0.f, sg = 0.f;
    bigru_for_valid_rows(lens, ty, rows, T, [&](int r) {
        const size_t e = (size_t)r * kBigruFc1 + c;
        const float dy = dbn[e];
        sb += dy;
        sg = fmaf(dy, (f1[e] * drop(e) - mean) * rstd, sg);
    });
    const double b = bigru_bn_lane_sum(red, sb, tx, ty);
    const double g = bigru_bn_lane_sum(red, sg, tx, ty);
    if (ty == 0) {
        dbeta[c] = (float)b;
        dgamma[c] = (float)g;
    }
}

// ... and the input gradient through the dropout in front of it, in place: d(fc1) = keep * gamma * rstd * (dy - dbeta / M - xhat * dgamma / M);
// zeros on padded rows
__global__ __launch_bounds__(256) void bigru_bn_bwd_dx_kernel(const float* __restrict__ f1, float* __restrict__ dbn, int rows, const BigruTapeHeader* hdr,
                                                              const int* __restrict__ tape_lens, const float* __restrict__ stats,
                                                              const float* __restrict__ gamma, const float* __restrict__ dgamma,
                                                              const float* __restrict__ dbeta) {
    const BigruDrop drop(hdr, kBigruSiteFc1);
    const int* const lens = bigru_tape_lens(hdr, tape_lens);
    const int T = hdr->T;
    const size_t n = (size_t)rows * kBigruFc1;
    const float inv_m = 1.f / (float)hdr->M;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        const int c = (int)(e % kBigruFc1);
        if (lens && !bigru_row_valid(lens, (int)(e / kBigruFc1), T)) {
            dbn[e] = 0.f;
            continue;
        }
        const float k = drop(e), rstd = stats[2 * kBigruFc1 + c];
        const float xhat = (f1[e] * k - stats[c]) * rstd;
        dbn[e] = k * gamma[c] * rstd * (dbn[e] - dbeta[c] * inv_m - xhat * dgamma[c] * inv_m);
    }
}

// ------------------------------------------------------------------------------------------------
// The backward recurrent sweep.
// ------------------------------------------------------------------------------------------------
// hprev[b, t] = forward half: y[b, t - 1] (zero at t = 0) | reverse half: y[b, t + 1] (zero at the sequence's last frame, t = len - 1): the
// A operand of dW_hh; zeros on padded rows
__global__ __launch_bounds__(256) void bigru_hprev_kernel(const float* __restrict__ y, float* __restrict__ hprev, int H, int T, long long n4,
                                                          const BigruTapeHeader* hdr, const int* __restrict__ tape_lens) {
    const int row4 = 2 * H / 4;
    const int* const lens = bigru_tape_lens(hdr, tape_lens);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const long long r = i / row4;
        const int c4 = (int)(i - r * row4), t = (int)(r % T);
        const int len = bigru_len(lens, (int)(r / T), T);
        const bool fwd = c4 < H / 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < len && (fwd ? t > 0 : t < len - 1)) v = reinterpret_cast<const float4*>(y)[i + (fwd ? -row4 : row4)];
        reinterpret_cast<float4*>(hprev)[i] = v;
    }
}

struct BigruRecBwdParams {
    const float* dy;     // [B * T][2H]: gradient of the layer's output (forward | reverse halves)
    const float* tape;   // [B * T][2][4H]: r | z | n | W_hn h + b_hn of every (frame, direction), kept by the forward sweep
    const float* y;      // [B * T][2H]: the layer's own output (h of the step before)
    const float4* wt;    // W_hh transposed, packed: [dir][third * CH + column][2H threads] float4 (bigru_pack_whh_kernel)
    float* dgx;          // [B * T][6H]: (da_r, da_z, da_n) in the forward's pre-gate layout: gradient of W_ih x + b_ih
    float* dgh;          // [B * T][6H]: (da_r, da_z, dq): gradient of W_hh h + b_hh
    int B, T;
    const BigruTapeHeader* hdr;
    const int* lens;     // the tape's frame counts (bigru_tape_lens): rows at or past a count are not read, and written as zeros in dgx / dgh
};

// One workgroup sweeps NS sequences of one direction from their last forward step to their first; nothing is shared between workgroups.
// Each sequence is swept over its own frame count (forward direction: frames len - 1 .. 0, reverse: 0 .. len - 1); the shorter one of a
// tile adds zeros once it is done, and every row from its count on gets zeros in dgx / dgh: that is what masks the GEMMs behind the sweep.
// Thread 2 j + q owns hidden unit j over half of the 3H-long k range of W_hh^T (da_r, da_z, dq): 3H / 2 weights, spread over registers, an LDS
// slab and an L2 stream as the forward's (BigruSplit).  (da_r, da_z, dq) of a step is double-buffered in LDS: one barrier per step.
template <int H, int NS>
__global__ __launch_bounds__(2 * H) void bigru_rec_bwd_kernel(const BigruRecBwdParams p) {
    using S = BigruSplit<H, NS>;
    constexpr int NT = S::NT, CH = S::CH, CR = S::CR, CL = S::CL, CG = S::CG;
    extern __shared__ float4 bigru_smem[];
    float4* const wl = bigru_smem;                                          // [3 * CL][NT]
    float* const vbuf = reinterpret_cast<float*>(bigru_smem + 3 * CL * NT);  // [2][NS][3H]
    const int tid = threadIdx.x, q = tid & 1, j = tid >> 1;
    const int dir = blockIdx.y, s0 = blockIdx.x * NS;
    const float4* const wd = p.wt + (size_t)dir * 3 * CH * NT;

    float4 wr[3][CR > 0 ? CR : 1];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int c = 0; c < CR; ++c) wr[g][c] = wd[(size_t)(g * CH + c) * NT + tid];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int c = 0; c < CL; ++c) wl[(g * CL + c) * NT + tid] = wd[(size_t)(g * CH + CR + c) * NT + tid];
    for (int k = tid; k < 2 * NS * 3 * H; k += NT) vbuf[k] = 0.f;
    __syncthreads();

    const int T = p.T;
    const int* const lens = bigru_tape_lens(p.hdr, p.lens);
    int len[NS], nmax = 0;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        len[s] = s0 + s < p.B ? bigru_len(lens, s0 + s, T) : 0;
        nmax = max(nmax, len[s]);
    }
    struct Step {
        float dy, r, z, n, q, hp;
    };
    auto load = [&](int s, int n, Step& v) {
        v.dy = v.r = v.z = v.n = v.q = v.hp = 0.f;
        if (n < len[s]) {
            const int f = dir == 0 ? len[s] - 1 - n : n;
            const size_t row = (size_t)(s0 + s) * T + f;
            v.dy = p.dy[row * (2 * H) + dir * H + j];
            const float* tp = p.tape + (row * 2 + dir) * (4 * H) + j;
            v.r = tp[0];
            v.z = tp[H];
            v.n = tp[2 * H];
            v.q = tp[3 * H];
            if (n + 1 < len[s]) v.hp = p.y[(dir == 0 ? row - 1 : row + 1) * (2 * H) + dir * H + j];
        }
    };

    float carry[NS], mv[NS];
    Step cur[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        carry[s] = mv[s] = 0.f;
        load(s, 0, cur[s]);
    }

    for (int n = 0; n < nmax; ++n) {
        Step nxt[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) load(s, n + 1, nxt[s]);
        float* const vn = vbuf + (n & 1) * NS * 3 * H;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const Step& v = cur[s];
            const float dh = (v.dy + carry[s]) + mv[s];
            const float dn = dh * (1.f - v.z), dz = dh * (v.hp - v.n);
            carry[s] = dh * v.z;
            const float dan = dn * (1.f - v.n * v.n), daz = dz * v.z * (1.f - v.z);
            const float dar = dan * v.q * v.r * (1.f - v.r), dq = dan * v.r;
            // (a sequence that is done: its Step is all zeros, so dar = daz = dq = 0 and carry stays 0; da_n is what W_hh^T leaves of its
            // first step and goes nowhere)
            if (q == 0) {
                vn[s * 3 * H + j] = dar;
                vn[s * 3 * H + H + j] = daz;
                vn[s * 3 * H + 2 * H + j] = dq;
                if (n < len[s]) {
                    const int f = dir == 0 ? len[s] - 1 - n : n;
                    const size_t o = ((size_t)(s0 + s) * T + f) * (6 * H) + (size_t)dir * 3 * H + j;
                    p.dgx[o] = dar;
                    p.dgx[o + H] = daz;
                    p.dgx[o + 2 * H] = dan;
                    p.dgh[o] = dar;
                    p.dgh[o + H] = daz;
                    p.dgh[o + 2 * H] = dq;
                }
            }
            cur[s] = nxt[s];
        }
        __syncthreads();  // step n's (da_r, da_z, dq) is complete; the buffer written two steps on was last read before this barrier's predecessor
        if (n + 1 == nmax) break;

        bigru_f2 acc[NS][3];
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int g = 0; g < 3; ++g) acc[s][g] = bigru_f2{0.f, 0.f};
        const float4* const v4 = reinterpret_cast<const float4*>(vn) + q * 3 * CH;
#pragma unroll
        for (int c = 0; c < CR; ++c)
#pragma unroll
            for (int s = 0; s < NS; ++s)
#pragma unroll
                for (int g = 0; g < 3; ++g) bigru_fma4(acc[s][g], wr[g][c], v4[s * (3 * H / 4) + g * CH + c]);
#pragma unroll
        for (int c = 0; c < CL; ++c) {
            float4 w[3];
#pragma unroll
            for (int g = 0; g < 3; ++g) w[g] = wl[(g * CL + c) * NT + tid];
#pragma unroll
            for (int s = 0; s < NS; ++s)
#pragma unroll
                for (int g = 0; g < 3; ++g) bigru_fma4(acc[s][g], w[g], v4[s * (3 * H / 4) + g * CH + CR + c]);
        }
#pragma unroll 4
        for (int c = 0; c < CG; ++c) {
            float4 w[3];
#pragma unroll
            for (int g = 0; g < 3; ++g) w[g] = wd[(size_t)(g * CH + CR + CL + c) * NT + tid];
#pragma unroll
            for (int s = 0; s < NS; ++s)
#pragma unroll
                for (int g = 0; g < 3; ++g) bigru_fma4(acc[s][g], w[g], v4[s * (3 * H / 4) + g * CH + CR + CL + c]);
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const float part = ((acc[s][0].x + acc[s][0].y) + (acc[s][1].x + acc[s][1].y)) + (acc[s][2].x + acc[s][2].y);
            mv[s] = part + __shfl_xor(part, 1);  // the two halves of the k range (commutative: both lanes get the same bits)
        }
    }
    // this direction's third of the padded rows of dgx / dgh: zeros (a dense tape has none)
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (s0 + s >= p.B) continue;
        const int w4 = 3 * H / 4;
        for (int k = tid; k < (T - len[s]) * w4; k += NT) {
            const size_t o = ((size_t)(s0 + s) * T + len[s] + k / w4) * (6 * H) + (size_t)dir * 3 * H + (size_t)(k % w4) * 4;
            *reinterpret_cast<float4*>(p.dgx + o) = make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(p.dgh + o) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
}

// W_hh of both directions (src: forward (3H, H), then reverse) in the recurrent kernels' orders:
//   fwd [dir][gate * H/8 + column][thread 2 i + q] float4 = W_hh[gate H + i][q H/2 + 4 column ..]              (as bigru_pack_whh on the host)
//   bwd [dir][third * H/8 + column][thread 2 j + q] float4 = W_hh[q 3H/2 + 4 (third H/8 + column) ..][j]       (the transpose's rows)
__global__ __launch_bounds__(256) void bigru_pack_whh_kernel(const float* __restrict__ src, float* __restrict__ fwd, float* __restrict__ bwd, int H) {
    const int NT = 2 * H, KH = H / 2, CH = KH / 4;
    const long long total = (long long)2 * 3 * CH * NT * 4;
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < total; k += (long long)gridDim.x * 256) {
        long long r = k;
        const int e = (int)(r & 3);
        r >>= 2;
        const int tid = (int)(r % NT);
        r /= NT;
        const int c = (int)(r % CH);
        r /= CH;
        const int gt = (int)(r % 3), dir = (int)(r / 3);
        const int i = tid >> 1, q = tid & 1;
        const float* w = src + (size_t)dir * 3 * H * H;
        fwd[k] = w[(size_t)(gt * H + i) * H + q * KH + 4 * c + e];
        bwd[k] = w[(size_t)(q * 3 * KH + (gt * CH + c) * 4 + e) * H + i];
    }
}

// fc1 with the eval-mode batch norm folded in, as hificar_bigru_finalize folds it on the host (same double arithmetic): wf (128, 2H), bf (128)
__global__ __launch_bounds__(256) void bigru_fold_fc1_kernel(const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, const float* __restrict__ mean, const float* __restrict__ var,
                                                             float* __restrict__ wf, float* __restrict__ bf, int cols) {
    const int o = blockIdx.x;
    const double s = (double)gamma[o] / sqrt((double)var[o] + 1e-5);
    for (int k = threadIdx.x; k < cols; k += 256) wf[(size_t)o * cols + k] = (float)((double)w[(size_t)o * cols + k] * s);
    if (threadIdx.x == 0) bf[o] = (float)(((double)b[o] - (double)mean[o]) * s + (double)beta[o]);
}

// rows [b * T + t][Cp] -> dx (B, C, T): the input gradient in the reference's layout
__global__ __launch_bounds__(256) void bigru_unrows_kernel(const float* __restrict__ rows, float* __restrict__ dx, int C, int Cp, int T) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z, c0 = blockIdx.y * 32, t0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const int t = t0 + r, c = c0 + tx;
        tile[r][tx] = (t < T && c < Cp) ? rows[((size_t)b * T + t) * Cp + c] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int c = c0 + r, t = t0 + tx;
        if (c < C && t < T) dx[((size_t)b * C + c) * T + t] = tile[tx][r];
    }
}

}  // namespace hificar
