// Weight-gradient GEMM for gfx950, register-staged kernel (fp32, and 16-bit types whose pixel rows are not 16-byte aligned):
//   dW[tap][o][i] = sum_pixels dy[pixel][o] * x[pix(pixel,tap)][i]
//
// The contraction index (pixels) is the SLOW index of both NHWC operands, so the MFMA
// fragments (8 consecutive k per lane) are formed with the CDNA4 transposing LDS read
// ds_read_b64_tr_b16 from row-major [pixel][channel] LDS images (16-bit types); the fp32
// path reads its one-k-per-lane fragments with plain ds_read_b32.
//  * tile BO x BI output, K step = 32 pixels (16-bit) / 16 pixels (fp32), 4 waves,
//    double-buffered register staging with one barrier per step (as igemm_staged_kernel.h);
//  * LDS rows are padded so that the 8 pixel rows a half-wave touches per transposed read
//    land on distinct bank groups; the k order inside a step is {4g..4g+3, 16+4g..16+4g+3}
//    for lane group g -- the same permutation for both operands, so the sum is unchanged;
//  * split-K over pixels -> fp32 slabs [split][tap][o][i], folded (deterministically, in
//    split order) into the reference-layout gradient by wgrad_reduce_kernel.
#pragma once
#include "wgrad_ring_kernel.h"     // WgradArgs

template <typename T> struct WFrag;

// 16-bit types: two transposed reads give the lane 8 k-values of one channel.
template <typename T> struct WFrag {
    static constexpr int KP = 32;
    static constexpr int PAD = 32;
    static __device__ __forceinline__ uint4 load(const unsigned char* tile, int rs, int ctile, int lane) {
        const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
        const unsigned char* a0 = tile + (4 * g + q) * rs + (ctile * 16 + 4 * pp) * 2;
        const unsigned char* a1 = a0 + 16 * rs;
        typedef s16x4 __attribute__((address_space(3))) * lds_p;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(a0));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(a1));
        union { struct { s16x4 l, h; } s; uint4 u; } r;
        r.s.l = lo; r.s.h = hi;
        return r.u;
    }
    static __device__ __forceinline__ void mma(const uint4& a, const uint4& b, f32x4& c);
};
template <> __device__ __forceinline__ void WFrag<bf16>::mma(const uint4& a, const uint4& b, f32x4& c) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
template <> __device__ __forceinline__ void WFrag<f16>::mma(const uint4& a, const uint4& b, f32x4& c) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// fp32: 16 pixels per step, instruction kk uses pixel 4*kk + (lane>>4).
template <> struct WFrag<float> {
    static constexpr int KP = 16;
    static constexpr int PAD = 64;
    static __device__ __forceinline__ uint4 load(const unsigned char* tile, int rs, int ctile, int lane) {
        const int g = lane >> 4, c = lane & 15;
        const unsigned char* a = tile + g * rs + (ctile * 16 + c) * 4;
        uint4 r;
        r.x = *reinterpret_cast<const unsigned*>(a);
        r.y = *reinterpret_cast<const unsigned*>(a + 4 * rs);
        r.z = *reinterpret_cast<const unsigned*>(a + 8 * rs);
        r.w = *reinterpret_cast<const unsigned*>(a + 12 * rs);
        return r;
    }
    static __device__ __forceinline__ void mma(const uint4& a, const uint4& b, f32x4& c) {
        const f32x4 fa = __builtin_bit_cast(f32x4, a), fb = __builtin_bit_cast(f32x4, b);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[0], fb[0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[1], fb[1], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[2], fb[2], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[3], fb[3], c, 0, 0, 0);
    }
};

template <typename T, int BO, int BI, int WO, int WI>
__global__ __launch_bounds__(256) void wgrad_kernel(const WgradArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int ES = sizeof(T);
    constexpr int EPC = 16 / ES;
    constexpr int KP = WFrag<T>::KP;
    constexpr int RSO = BO * ES + WFrag<T>::PAD, RSI = BI * ES + WFrag<T>::PAD;
    constexpr int CPO = BO * ES / 16, CPI = BI * ES / 16;     // chunks per pixel row
    constexpr int NO = KP * CPO / 256, NI = KP * CPI / 256;   // chunks per thread and step
    constexpr int STAGE = KP * (RSO + RSI);
    constexpr int TO = BO / WO, TI = BI / WI, OT = TO / 16, IT = TI / 16;
    static_assert(WO * WI == 4 && NO >= 1 && NI >= 1, "bad tile");

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wo_ = wave / WI, wi_ = wave % WI;
    const int otile = blockIdx.x / p.i_tiles, itile = blockIdx.x % p.i_tiles;
    const int tap = blockIdx.y, split = blockIdx.z;
    const int dh = p.dh[tap], dw = p.dw[tap];
    const int hw = p.ho * p.wo;
    const long m_begin = (long)split * p.steps_per_split * KP;
    long m_end = m_begin + (long)p.steps_per_split * KP;
    if (m_end > p.M) m_end = p.M;
    const int S = m_begin < m_end ? (int)((m_end - m_begin + KP - 1) / KP) : 0;

    f32x4 acc[OT][IT];
#pragma unroll
    for (int i = 0; i < OT; ++i)
#pragma unroll
        for (int j = 0; j < IT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int orow = tid / CPO, ochunk = tid % CPO;
    const int irow = tid / CPI, ichunk = tid % CPI;
    const int ocol = otile * BO + ochunk * EPC, icol = itile * BI + ichunk * EPC;
    uint4 ro[NO], ri[NI];

    auto gload = [&](int s) {
        const long mb = m_begin + (long)s * KP;
#pragma unroll
        for (int i = 0; i < NO; ++i) {
            const long m = mb + orow + i * (256 / CPO);
            if (m < m_end && ocol < p.n_out)
                ro[i] = *reinterpret_cast<const uint4*>(p.dy + (m * p.dy_pix_stride + ocol) * ES);
            else
                ro[i] = uint4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const long m = mb + irow + i * (256 / CPI);
            bool ok = m < m_end && icol < p.k_run;
            long e = 0;
            if (ok) {
                const int mi = (int)m;
                const int n = mi / hw, rem = mi - n * hw;
                const int a = rem / p.wo, b = rem - a * p.wo;
                const int ih = a * p.sh + dh, iw = b * p.sw + dw;
                ok = (unsigned)ih < (unsigned)p.hi && (unsigned)iw < (unsigned)p.wi;
                e = ((long)(n * p.hi + ih) * p.wi + iw) * p.in_pix_stride + icol;
            }
            ri[i] = ok ? *reinterpret_cast<const uint4*>(p.x + e * ES) : uint4{0u, 0u, 0u, 0u};
        }
    };

    if (S > 0) gload(0);
    for (int s = 0; s < S; ++s) {
        unsigned char* so = smem + (s & 1) * STAGE;
        unsigned char* si = so + KP * RSO;
#pragma unroll
        for (int i = 0; i < NO; ++i)
            *reinterpret_cast<uint4*>(so + (orow + i * (256 / CPO)) * RSO + ochunk * 16) = ro[i];
#pragma unroll
        for (int i = 0; i < NI; ++i)
            *reinterpret_cast<uint4*>(si + (irow + i * (256 / CPI)) * RSI + ichunk * 16) = ri[i];
        __syncthreads();
        if (s + 1 < S) gload(s + 1);
        uint4 fo[OT], fi[IT];
#pragma unroll
        for (int i = 0; i < OT; ++i) fo[i] = WFrag<T>::load(so, RSO, wo_ * OT + i, lane);
#pragma unroll
        for (int j = 0; j < IT; ++j) fi[j] = WFrag<T>::load(si, RSI, wi_ * IT + j, lane);
#pragma unroll
        for (int i = 0; i < OT; ++i)
#pragma unroll
            for (int j = 0; j < IT; ++j) WFrag<T>::mma(fo[i], fi[j], acc[i][j]);
    }

    float* slab = p.slab + ((long)split * p.ntaps + tap) * p.n_out * p.n_in;
    const int q = lane >> 4, c = lane & 15;
#pragma unroll
    for (int i = 0; i < OT; ++i)
#pragma unroll
        for (int j = 0; j < IT; ++j) {
            const int ci = itile * BI + wi_ * TI + j * 16 + c;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = otile * BO + wo_ * TO + i * 16 + q * 4 + r;
                if (o < p.n_out && ci < p.n_in) slab[(long)o * p.n_in + ci] = acc[i][j][r];
            }
        }
}
