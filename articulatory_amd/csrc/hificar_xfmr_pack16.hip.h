// The two element-wise passes of the Transformer's bf16x3 training arithmetic (hificar_xfmr_set_train_precision):
//   pack16_kernel        a device fp32 weight in the reference's layout -> the bf16 hi | lo fragments pack_w16 (hificar.hip) builds on the host,
//                        byte for byte: the weights change every step, so the fragments are rebuilt on the device, on the step's stream
//   xfmr_split_rows_kernel   fp32 rows -> split rows [hi: C bf16 | lo: C bf16], the bf16x3 GEMMs' input format (xfmr_store_split)
// The pack's index arithmetic is plain C++ (HIFICAR_HD functions): the library runs the same functions on the host for the test of the map
// (hificar_debug_pack16, mode "host").
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define HIFICAR_HD __host__ __device__ __forceinline__
#else
#define HIFICAR_HD inline
#endif

namespace hificar {

constexpr int kPack16MaxTaps = 16;

// fragments: [n_block32][chunk][tap][c16][hi | lo][lane][8] bf16, + a zero tail of 4 nc16 fragments (the engine's weight prefetch runs past the end)
struct Pack16Params {
    const float* src;  // mode 0: (cout, cin, K) as stored;  mode 2: the same tensor, packed as its data gradient's Conv1d:
                       //         w'[co' = ci][ci' = co][t] = W[co][ci][K - 1 - t]
    uint16_t* dst;
    int mode;
    int n_blocks32, nchunk, ntaps, nc16, chunk;
    int cin, cout, K;         // of the SOURCE weight
    int cin_pack, cout_pack;  // real input / output channels of the packed layer (mode 2: cout, cin of the source)
    int tap_k[kPack16MaxTaps];  // kernel index of the packed layer's tap t; < 0: zero weights
};

// one work item = one lane's eight channels of one (block, chunk, 16-channel slab), all taps
HIFICAR_HD long long pack16_items(const Pack16Params& p) { return (long long)p.n_blocks32 * p.nchunk * p.nc16 * 64; }
// fragments in front of the zero tail, and with it (in bf16 elements: x 512)
HIFICAR_HD long long pack16_frags(const Pack16Params& p) { return (long long)p.n_blocks32 * p.nchunk * p.ntaps * p.nc16 * 2; }

struct Pack16Item {
    int nb, c, u, lane;
    int co, ci0;  // the lane's output channel and the first of its eight input channels, of the packed layer
};

HIFICAR_HD Pack16Item pack16_decode(const Pack16Params& p, long long i) {
    Pack16Item it;
    it.lane = (int)(i & 63);
    long long r = i >> 6;
    it.u = (int)(r % p.nc16);
    r /= p.nc16;
    it.c = (int)(r % p.nchunk);
    it.nb = (int)(r / p.nchunk);
    it.co = it.nb * 32 + (it.lane & 31);
    it.ci0 = it.c * p.chunk + it.u * 16 + 8 * (it.lane >> 5);
    return it;
}

// index into src of (packed output channel co, packed input channel ci, packed tap t); -1: the element is zero
HIFICAR_HD long long pack16_src_index(const Pack16Params& p, int co, int ci, int t) {
    const int k = p.tap_k[t];
    if (k < 0 || k >= p.K || co >= p.cout_pack || ci >= p.cin_pack) return -1;
    if (p.mode == 0) return ((long long)co * p.cin + ci) * p.K + k;
    return ((long long)ci * p.cin + co) * p.K + (p.K - 1 - k);
}

// bf16 element offset of the lane's eight hi values of tap t (the lo values: + 512)
HIFICAR_HD long long pack16_dst_index(const Pack16Params& p, const Pack16Item& it, int t) {
    return ((((((long long)it.nb * p.nchunk + it.c) * p.ntaps + t) * p.nc16 + it.u) * 2) * 64 + it.lane) * 8;
}

HIFICAR_HD uint16_t pack16_bf16(float f) {  // round to nearest even (finite inputs): pack_w16's f32_to_bf16
    uint32_t u;
    memcpy(&u, &f, 4);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
HIFICAR_HD float pack16_f32(uint16_t b) {
    const uint32_t u = (uint32_t)b << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// one item: reads its 8 x ntaps source values, writes 2 x ntaps runs of 16 bytes
HIFICAR_HD void pack16_item(const Pack16Params& p, long long i) {
    const Pack16Item it = pack16_decode(p, i);
    for (int t = 0; t < p.ntaps; ++t) {
        alignas(16) uint16_t hi[8], lo[8];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int j = 0; j < 8; ++j) {
            const long long s = pack16_src_index(p, it.co, it.ci0 + j, t);
            const float v = s >= 0 ? p.src[s] : 0.f;
            hi[j] = pack16_bf16(v);
            lo[j] = pack16_bf16(v - pack16_f32(hi[j]));
        }
        uint16_t* const d = p.dst + pack16_dst_index(p, it, t);
        memcpy(d, hi, 16);
        memcpy(d + 512, lo, 16);
    }
}

#if defined(__HIPCC__)
// the zero tail is written too (4 nc16 fragments of 512 bf16 = 256 nc16 runs of 16 bytes): what the buffer held before does not matter
__global__ __launch_bounds__(256) void pack16_kernel(const Pack16Params p) {
    const long long n = pack16_items(p), step = (long long)gridDim.x * 256, first = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p.ntaps == 1 && p.mode == 0 && p.K == 1 && (p.cin & 7) == 0 && p.tap_k[0] == 0) {
        // a Linear as stored: the lane's eight values are 32 adjacent bytes of the source
        for (long long i = first; i < n; i += step) {
            const Pack16Item it = pack16_decode(p, i);
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
            if (it.co < p.cout_pack && it.ci0 < p.cin_pack) {  // (8 | cin: all eight or none)
                const float4* const s = reinterpret_cast<const float4*>(p.src + (size_t)it.co * p.cin + it.ci0);
                a = s[0];
                b = s[1];
            }
            const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            uint32_t H[4], L[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint16_t h0 = pack16_bf16(v[2 * j]), h1 = pack16_bf16(v[2 * j + 1]);
                const uint16_t l0 = pack16_bf16(v[2 * j] - pack16_f32(h0)), l1 = pack16_bf16(v[2 * j + 1] - pack16_f32(h1));
                H[j] = (uint32_t)h0 | ((uint32_t)h1 << 16);
                L[j] = (uint32_t)l0 | ((uint32_t)l1 << 16);
            }
            uint16_t* const d = p.dst + pack16_dst_index(p, it, 0);
            *reinterpret_cast<uint4*>(d) = make_uint4(H[0], H[1], H[2], H[3]);
            *reinterpret_cast<uint4*>(d + 512) = make_uint4(L[0], L[1], L[2], L[3]);
        }
    } else {
        for (long long i = first; i < n; i += step) pack16_item(p, i);
    }
    uint4* const tail = reinterpret_cast<uint4*>(p.dst + pack16_frags(p) * 512);
    for (long long i = first; i < 256LL * p.nc16; i += step) tail[i] = make_uint4(0u, 0u, 0u, 0u);
}

// fp32 rows [M][C] -> split rows [M][hi: C bf16 | lo: C bf16] (8 | C): a lane reads eight adjacent channels (two 16-byte loads) and writes 16
// bytes of the hi half and 16 of the lo half.  hi = bf16(x), lo = bf16(x - hi), round to nearest even: xfmr_store_split's expression.
// The rows of padded frames (ragged tape) and the gap rows (packed) are written as zero bits and not read.  n8 = M C / 8.
__global__ __launch_bounds__(256) void xfmr_split_rows_kernel(const float* __restrict__ x, char* __restrict__ rows, long long n8, int C,
                                                              const BigruTapeHeader* hdr, const int* __restrict__ tape_lens, int T, const XfmrLayout lay) {
    const int* const lens = bigru_tape_lens(hdr, tape_lens);
    const int c8n = C >> 3;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
        const long long r = i / c8n;
        const int c = (int)(i - r * c8n) * 8;
        bf16x8 hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) hi[e] = lo[e] = (__bf16)0.f;
        if (xfmr_elem_valid(lay, lens, r * C, C, T)) {
            const float4 a = *reinterpret_cast<const float4*>(x + r * C + c), b = *reinterpret_cast<const float4*>(x + r * C + c + 4);
            const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                hi[e] = (__bf16)v[e];
                lo[e] = (__bf16)(v[e] - (float)hi[e]);
            }
        }
        char* const row = rows + (size_t)r * C * 4;
        *reinterpret_cast<bf16x8*>(row + 2 * c) = hi;
        *reinterpret_cast<bf16x8*>(row + 2 * C + 2 * c) = lo;
    }
}
#endif

}  // namespace hificar
