// Device-only helpers of the MGPIS kernels that more than one kernel family uses (the SELL kernels
// of device_mgpis.hip, the colour sweeps, the transfers, the PCG recurrence and the setup): the
// chunk partial, the stop flag, the smoother inverse, the x gathers and the 3x3 block product over
// every storage type, the slot loop.  Included by the device_mgpis*.hip sources only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "device_mgpis.hpp"

namespace ddpca {
namespace {

// Chunk partial of a dot product: one wavefront = one 64-node chunk, fixed shuffle order.
__device__ __forceinline__ void chunk_partial(double v, double* partial, int64_t chunk) {
    v = wsum(v);
    if ((threadIdx.x & 63) == 0) partial[chunk] = v;
}

__device__ __forceinline__ bool stopped(const PcgScal* sc, int sub) { return sc && sc[sub].done; }

template <bool BJ, typename MT = double>
__device__ __forceinline__ void apply_m(const MT* minv, int64_t row, double r0, double r1, double r2,
                                        double& m0, double& m1, double& m2) {
    if (BJ) {
        const MT* m = minv + 9 * row;
        m0 = __builtin_fma((double)m[2], r2, __builtin_fma((double)m[1], r1, (double)m[0] * r0));
        m1 = __builtin_fma((double)m[5], r2, __builtin_fma((double)m[4], r1, (double)m[3] * r0));
        m2 = __builtin_fma((double)m[8], r2, __builtin_fma((double)m[7], r1, (double)m[6] * r0));
    } else {
        const MT* m = minv + 3 * row;
        m0 = m[0] * r0;
        m1 = m[1] * r1;
        m2 = m[2] * r2;
    }
}

// (the value layout of a slot in each storage type, slot_elem / slot_vals: mgpis_layout.hpp)
typedef double dbl2_t __attribute__((ext_vector_type(2)));

// storage type of the smoother inverse on a level whose operator values are stored as T: fp64
// with fp64 operators, fp32 on the reduced-precision levels (precond_fp32 >= 1)
template <typename T>
using SmoothInv = typename std::conditional<sizeof(T) == 8, double, float>::type;

__device__ __forceinline__ double h16_lo(uint32_t w) {
    return (double)__builtin_bit_cast(_Float16, (uint16_t)(w & 0xFFFFu));
}
__device__ __forceinline__ double h16_hi(uint32_t w) { return (double)__builtin_bit_cast(_Float16, (uint16_t)(w >> 16)); }

// x_j gathered for a block product: three fp64 values at stride 3 (three 8-B loads), or -- the
// multicolour sweeps' fp32 iterate copy (GsFine::x4, precond_fp32 = 4) -- one 16-B load of the
// node's (x0, x1, x2, 0) in fp32, widened to fp64
struct X3 {
    double a, b, c;
};
__device__ __forceinline__ X3 ldx(const double* x, int64_t j) { return X3{x[3 * j], x[3 * j + 1], x[3 * j + 2]}; }
__device__ __forceinline__ X3 ldx(const float4* x, int64_t j) {
    const float4 v = x[j];
    return X3{(double)v.x, (double)v.y, (double)v.z};
}

// 3x3 block times x_j, accumulated in fp64; v = slot base + lane.  The matrix is streamed once
// per launch (NT: non-temporal loads, leaving the caches to the x gathers).
template <bool NT, typename T>
__device__ __forceinline__ void block_fma_any(const T* v, X3 xj, double& s0, double& s1, double& s2, int lane) {
    const double x0 = xj.a, x1 = xj.b, x2 = xj.c;
    auto ldv = [](const auto* p) { if constexpr (NT) return __builtin_nontemporal_load(p); else return *p; };
    // row . x as fma(v2, x2, fma(v1, x1, v0 x0)), added to the accumulator: the contraction is
    // spelled out so every kernel instantiating this rounds alike (left to fp-contract, the
    // compiler fused different products in different kernels, e.g. the colour sweeps over
    // column-indexed and stencil-coded slots)
    auto dot3 = [x0, x1, x2](double v0, double v1, double v2) { return __builtin_fma(v2, x2, __builtin_fma(v1, x1, v0 * x0)); };
    if constexpr (sizeof(T) == 1) {
        // v = slot base + lane in bytes; the lane's dwords at 4 lane, 256 + 4 lane, 512 + 4 lane
        const uint32_t* p = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(v) - lane) + lane;
        const uint32_t a = ldv(p), b = ldv(p + 64), c = ldv(p + 128);
        auto q = [](uint32_t w, int k) { return (double)((int32_t)(w << (24 - 8 * k)) >> 24); };  // signed byte k
        const double sc = (double)__builtin_bit_cast(float, c & 0xFFFFFF00u);
        s0 = __builtin_fma(sc, dot3(q(a, 0), q(a, 1), q(a, 2)), s0);
        s1 = __builtin_fma(sc, dot3(q(a, 3), q(b, 0), q(b, 1)), s1);
        s2 = __builtin_fma(sc, dot3(q(b, 2), q(b, 3), q(c, 0)), s2);
    } else if constexpr (sizeof(T) == 2) {
        // v = slot base + lane in halves; the lane's dword of pair p is at dword 64 p + lane
        const uint32_t* p = reinterpret_cast<const uint32_t*>(v - lane) + lane;
        const uint32_t a = ldv(p), b = ldv(p + 64), c = ldv(p + 128), d = ldv(p + 192), e = ldv(p + 256);
        const double sc = __builtin_amdgcn_ldexp(1.0, (int)(int16_t)(e >> 16));
        s0 = __builtin_fma(sc, dot3(h16_lo(a), h16_hi(a), h16_lo(b)), s0);
        s1 = __builtin_fma(sc, dot3(h16_hi(b), h16_lo(c), h16_hi(c)), s1);
        s2 = __builtin_fma(sc, dot3(h16_lo(d), h16_hi(d), h16_lo(e)), s2);
    } else if constexpr (paired_values<T>() && sizeof(T) == 8) {
        const dbl2_t* p = reinterpret_cast<const dbl2_t*>(v - lane) + lane;
        const dbl2_t a = ldv(p), b = ldv(p + 64), c = ldv(p + 128), d = ldv(p + 192);
        const double v8 = ldv(v + 512);
        s0 = s0 + dot3(a.x, a.y, b.x);
        s1 = s1 + dot3(b.y, c.x, c.y);
        s2 = s2 + dot3(d.x, d.y, v8);
    } else {
        auto ld = [&](int i) { return (double)ldv(v + i * kChunk); };
        s0 = s0 + dot3(ld(0), ld(1), ld(2));
        s1 = s1 + dot3(ld(3), ld(4), ld(5));
        s2 = s2 + dot3(ld(6), ld(7), ld(8));
    }
}

template <typename T>
__device__ __forceinline__ void block_fma(const T* v, X3 xj, double& s0, double& s1, double& s2) {
    block_fma_any<true>(v, xj, s0, s1, s2, threadIdx.x & 63);
}

template <typename T>
__device__ __forceinline__ void block_fma_plain(const T* v, X3 xj, double& s0, double& s1, double& s2) {
    block_fma_any<false>(v, xj, s0, s1, s2, threadIdx.x & 63);
}

// Row sums of one chunk, loop variant V (the production kernels use default_variant; the others
// are kept for mgpis_gpu_bench_spmv, which times them on a live operator):
//   0  slot loop unrolled x3, cached loads
//   1  as 0 with non-temporal matrix loads
//   2  groups of 3 slots with the next group's columns prefetched, non-temporal matrix loads
// Column of slot k for this lane: CT = int32_t holds the block column, CT = int16_t its offset
// from the row's own node (col16: every |column - row| of the level < 2^15, which the
// lexicographic device numbering gives for subdomains up to ~180 x 180 nodes per plane) --
// 2 B instead of 4 per block.
template <typename CT>
__device__ __forceinline__ int64_t col_of(CT c, int64_t row) {
    if constexpr (sizeof(CT) == 2) return row + (int64_t)c;
    else return (int64_t)c;
}

// slot-loop unroll of the sweeps gathering an fp32 iterate copy (colour sweeps, block-Jacobi
// levels; A/B builds: -DDDPCA_GS_UNROLL=n)
#ifndef DDPCA_GS_UNROLL
#define DDPCA_GS_UNROLL 3
#endif
constexpr int kGsUnroll = DDPCA_GS_UNROLL;

template <int V, typename T, typename CT = int32_t, typename XT = double, int U = 3>
__device__ __forceinline__ void sell_rows(const CT* colp, const T* valp, const XT* x, int ns, int64_t row,
                                          double& s0, double& s1, double& s2) {
    constexpr int64_t SV = slot_vals<T>() * kChunk;
    if constexpr (V == 0) {
#pragma unroll 3
        for (int k = 0; k < ns; ++k)
            block_fma_plain(valp + (int64_t)k * SV, ldx(x, col_of(colp[(int64_t)k * kChunk], row)), s0, s1, s2);
    } else if constexpr (V == 1) {
#pragma unroll U
        for (int k = 0; k < ns; ++k)
            block_fma(valp + (int64_t)k * SV, ldx(x, col_of(__builtin_nontemporal_load(colp + (int64_t)k * kChunk), row)),
                      s0, s1, s2);
    } else if constexpr (V == 3) {
        // diagnostic bound only (wrong product): as 1 but x gathered at the row's own node, i.e.
        // perfectly coalesced gathers -- what a locality-optimal node numbering could approach
#pragma unroll 3
        for (int k = 0; k < ns; ++k) {
            const int64_t j = col_of(__builtin_nontemporal_load(colp + (int64_t)k * kChunk), row);
            block_fma(valp + (int64_t)k * SV, ldx(x, row + (j & 0)), s0, s1, s2);
        }
    } else {
        int k = 0;
        CT c0 = 0, c1 = 0, c2 = 0;
        if (ns >= 3) {
            c0 = __builtin_nontemporal_load(colp);
            c1 = __builtin_nontemporal_load(colp + kChunk);
            c2 = __builtin_nontemporal_load(colp + 2 * kChunk);
        }
        for (; k + 3 <= ns; k += 3) {
            const int64_t j0 = col_of(c0, row), j1 = col_of(c1, row), j2 = col_of(c2, row);
            if (k + 6 <= ns) {
                c0 = __builtin_nontemporal_load(colp + (int64_t)(k + 3) * kChunk);
                c1 = __builtin_nontemporal_load(colp + (int64_t)(k + 4) * kChunk);
                c2 = __builtin_nontemporal_load(colp + (int64_t)(k + 5) * kChunk);
            }
            const T* v = valp + (int64_t)k * SV;
            block_fma(v, ldx(x, j0), s0, s1, s2);
            block_fma(v + SV, ldx(x, j1), s0, s1, s2);
            block_fma(v + 2 * SV, ldx(x, j2), s0, s1, s2);
        }
        for (; k < ns; ++k) block_fma(valp + (int64_t)k * SV, ldx(x, col_of(colp[(int64_t)k * kChunk], row)), s0, s1, s2);
    }
}

// Node-parallel kernels: thread = node, 256 nodes per workgroup; a wavefront is one chunk, so
// the subdomain (and its stop flag) is uniform per wavefront.  nn is a multiple of 64.
#define NODE_PROLOGUE(nn, csub, sc)                         \
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; \
    if (i >= (nn)) return;                                  \
    const int sub = (csub)[i >> 6];                         \
    if (stopped((sc), sub)) return;

}  // namespace
}  // namespace ddpca
