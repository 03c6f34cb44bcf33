// Weight packs for the implicit-GEMM kernels: one tensor, all of a model in one launch, and the tiled transposing pack.
#include "common.h"

// ------------------------------------------------------------------------------------------------ weight pack
struct PackArgs {
    const float* w;
    void* out;
    int n_out, n_in, ntaps, kpad, rows;
    long so, si, sr, ss;
    signed char r[64];
    signed char s[64];
};

template <typename T>
__global__ void pack_weight_kernel(const PackArgs p) {
    const long total = (long)p.rows * p.ntaps * p.kpad;
    T* out = (T*)p.out;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int k = (int)(i % p.kpad);
        const long t2 = i / p.kpad;
        const int t = (int)(t2 % p.ntaps), o = (int)(t2 / p.ntaps);
        float v = 0.f;
        if (o < p.n_out && k < p.n_in) v = p.w[o * p.so + k * p.si + p.r[t] * p.sr + p.s[t] * p.ss];
        out[i] = from_f<T>(v);
    }
}

extern "C" int lh_pack_weight(const float* w, void* out, size_t* bytes, int n_out, int n_in, long so, long si,
                              long sr, long ss, int ntaps, const int* taps_rs, int dtype, void* stream) {
    const int es = lh_dtype_size(dtype);
    LH_REQUIRE(es > 0, "lh_pack_weight: bad dtype %d", dtype);
    LH_REQUIRE(n_out > 0 && n_in > 0 && ntaps >= 0 && ntaps <= 64, "lh_pack_weight: bad sizes");
    const int kstep = 128 / es;          // K is padded to the 128-byte step of the ring kernel
    const int kpad = (n_in + kstep - 1) / kstep * kstep;
    const int rows = (n_out + 127) / 128 * 128;
    const size_t need = (size_t)rows * (ntaps > 0 ? ntaps : 1) * kpad * es;
    if (bytes) *bytes = need;
    if (!out) return LH_OK;
    if (ntaps == 0) return LH_OK;
    LH_REQUIRE(w && taps_rs, "lh_pack_weight: null pointer");
    PackArgs a;
    a.w = w; a.out = out; a.n_out = n_out; a.n_in = n_in; a.ntaps = ntaps; a.kpad = kpad; a.rows = rows;
    a.so = so; a.si = si; a.sr = sr; a.ss = ss;
    for (int t = 0; t < 64; ++t) {
        a.r[t] = t < ntaps ? (signed char)taps_rs[2 * t] : 0;
        a.s[t] = t < ntaps ? (signed char)taps_rs[2 * t + 1] : 0;
    }
    const long total = (long)rows * ntaps * kpad;
    const int grid = lh_grid(total, 4096);
    LH_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((pack_weight_kernel<T>), dim3(grid), dim3(256), 0, (hipStream_t)stream, a));
    LH_LAUNCH_CHECK("pack_weight launch");
    return LH_OK;
}

// All packs of a model in ONE launch: the host cuts every pack into chunks of PACK_CHUNK output elements and
// blockIdx.x walks the chunk table (device arrays), so big and small packs are balanced over the grid.
constexpr int PACK_CHUNK = 2048;         // elements per workgroup: 8 dependent gathers per thread (the stem pack is 57k elements: 28 workgroups, not 2)

template <typename T>
__global__ __launch_bounds__(256) void pack_weight_multi_kernel(const lh_pack_item* items, const int* chunk_item,
                                                                const long* chunk_start) {
    const lh_pack_item& p = items[chunk_item[blockIdx.x]];
    const int es = sizeof(T);
    const int kstep = 128 / es;
    const int kpad = (p.n_in + kstep - 1) / kstep * kstep;
    const int rows = (p.n_out + 127) / 128 * 128;
    const long total = (long)rows * p.ntaps * kpad;
    const long begin = chunk_start[blockIdx.x];
    long end = begin + PACK_CHUNK;
    if (end > total) end = total;
    T* out = (T*)p.out;
    for (long i = begin + threadIdx.x; i < end; i += 256) {
        const int k = (int)(i % kpad);
        const long t2 = i / kpad;
        const int t = (int)(t2 % p.ntaps), o = (int)(t2 / p.ntaps);
        float v = 0.f;
        if (o < p.n_out && k < p.n_in) v = p.w[o * p.so + k * p.si + p.r[t] * p.sr + p.s[t] * p.ss];
        out[i] = from_f<T>(v);
    }
}

extern "C" int lh_pack_chunk_elems(void) { return PACK_CHUNK; }

extern "C" int lh_pack_weights_multi(const lh_pack_item* items_dev, const int* chunk_item_dev, const long* chunk_start_dev,
                                     int n_chunks, int dtype, void* stream) {
    LH_REQUIRE(items_dev && chunk_item_dev && chunk_start_dev && n_chunks > 0, "lh_pack_weights_multi: bad arguments");
    LH_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((pack_weight_multi_kernel<T>), dim3(n_chunks), dim3(256), 0, (hipStream_t)stream,
                                                   items_dev, chunk_item_dev, chunk_start_dev));
    LH_LAUNCH_CHECK("pack_weights_multi launch");
    return LH_OK;
}

// Transposing pack for regular weight tensors w[d0][d1][rs] (Conv2d: d0 = C_out, d1 = C_in; ConvTranspose2d:
// d0 = C_in, d1 = C_out): one workgroup reads a 32 x 32 x rs tile with fully coalesced loads (the strided
// per-element gather of pack_weight_multi_kernel over-fetches ~16x, profiles/r01_pmc_hbm_traffic.txt), keeps it in
// LDS and writes every pack that needs it -- "row = d0" packs [d0][tap][d1] and "row = d1" packs [d1][tap][d0] --
// in 64-byte runs.  Pack padding (rows >= n, K >= n_in) is zeroed once at allocation and never written.
template <typename T>
__global__ __launch_bounds__(256) void pack_tiled_kernel(const lh_pack_conv* convs, const int* chunk_conv, const int* chunk_t0,
                                                         const int* chunk_t1) {
    extern __shared__ __attribute__((aligned(16))) unsigned char psm[];
    T* tile = reinterpret_cast<T*>(psm);                         // [32 d0][32 d1][rs] (+4 pad per d0 row)
    const lh_pack_conv& c = convs[chunk_conv[blockIdx.x]];
    const int t0 = chunk_t0[blockIdx.x] * 32, t1 = chunk_t1[blockIdx.x] * 32;
    const int rs = c.rs;
    const int rowlen = 32 * rs;                                  // contiguous floats per d0 row of the tile
    const int ld = rowlen + 4;                                   // LDS row stride in elements (8-byte aligned rows)
    const bool full = t0 + 32 <= c.d0 && t1 + 32 <= c.d1 && ((long)c.d1 * rs) % 4 == 0 && sizeof(T) == 2;
    if (full) {                                                  // interior tile: 16-byte loads, 8-byte LDS stores
        const int vpr = rowlen / 4;                              // float4 per row
        for (int i = threadIdx.x; i < 32 * vpr; i += 256) {
            const int a = i / vpr, v4 = i - a * vpr;
            const float4 v = *reinterpret_cast<const float4*>(c.w + ((long)(t0 + a) * c.d1 + t1) * rs + v4 * 4);
            union { uint2 u; T e[4]; } pk;
            pk.e[0] = from_f<T>(v.x); pk.e[1] = from_f<T>(v.y); pk.e[2] = from_f<T>(v.z); pk.e[3] = from_f<T>(v.w);
            *reinterpret_cast<uint2*>(tile + a * ld + v4 * 4) = pk.u;
        }
    } else {
        for (int i = threadIdx.x; i < 32 * rowlen; i += 256) {
            const int a = i / rowlen, rem = i - a * rowlen;      // a = d0 offset, rem = d1_off * rs + tap
            const int d0 = t0 + a, d1 = t1 + rem / rs;
            float v = 0.f;
            if (d0 < c.d0 && d1 < c.d1) v = c.w[((long)d0 * c.d1 + t1) * rs + rem];
            tile[a * ld + rem] = from_f<T>(v);
        }
    }
    __syncthreads();
    for (int p = 0; p < c.npacks; ++p) {
        const lh_pack_out& o = c.packs[p];
        T* out = reinterpret_cast<T*>(o.out);
        const int nrow = o.row_is_d1 ? c.d1 : c.d0, nk = o.row_is_d1 ? c.d0 : c.d1;
        const int r0 = o.row_is_d1 ? t1 : t0, k0 = o.row_is_d1 ? t0 : t1;
        if (full && (o.kpad & 3) == 0) {                         // four K values per thread: one 8-byte store
            const int total = o.ntaps * 32 * 8;
            for (int i = threadIdx.x; i < total; i += 256) {
                const int k = (i & 7) * 4, rest = i >> 3;
                const int t = rest % o.ntaps, row = rest / o.ntaps;
                const int tap = o.taps[t];
                union { uint2 u; T e[4]; } pk;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    pk.e[e] = o.row_is_d1 ? tile[(k + e) * ld + row * rs + tap] : tile[row * ld + (k + e) * rs + tap];
                *reinterpret_cast<uint2*>(out + ((long)(r0 + row) * o.ntaps + t) * o.kpad + k0 + k) = pk.u;
            }
            continue;
        }
        const int total = o.ntaps * 32 * 32;
        for (int i = threadIdx.x; i < total; i += 256) {
            const int k = i & 31, rest = i >> 5;                 // k runs along the pack's K (fastest in memory)
            const int t = rest % o.ntaps, row = rest / o.ntaps;
            const int tap = o.taps[t];
            int a, b;                                            // a = d0 offset, b = d1 offset inside the tile
            if (o.row_is_d1) { b = row; a = k; } else { a = row; b = k; }
            const int grow = r0 + row, gk = k0 + k;
            if (grow < nrow && gk < nk) out[((long)grow * o.ntaps + t) * o.kpad + gk] = tile[a * ld + b * rs + tap];
        }
    }
}

extern "C" int lh_pack_weights_tiled(const lh_pack_conv* convs_dev, const int* chunk_conv_dev, const int* chunk_t0_dev,
                                     const int* chunk_t1_dev, int n_chunks, int max_rs, int dtype, void* stream) {
    LH_REQUIRE(convs_dev && chunk_conv_dev && chunk_t0_dev && chunk_t1_dev && n_chunks > 0 && max_rs > 0 && max_rs <= 49,
               "lh_pack_weights_tiled: bad arguments");
    const int es = lh_dtype_size(dtype);
    const size_t lds = (size_t)32 * (32 * max_rs + 4) * es;
    LH_REQUIRE(lds <= 64 * 1024, "lh_pack_weights_tiled: tile of %d taps does not fit LDS for this dtype", max_rs);
    LH_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((pack_tiled_kernel<T>), dim3(n_chunks), dim3(256), lds, (hipStream_t)stream,
                                                   convs_dev, chunk_conv_dev, chunk_t0_dev, chunk_t1_dev));
    LH_LAUNCH_CHECK("pack_weights_tiled launch");
    return LH_OK;
}
