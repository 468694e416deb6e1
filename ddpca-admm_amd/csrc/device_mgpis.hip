// MGPIS device path: SELL-BSR3 kernels, V-cycle and PCG for gfx950 over a batch of
// subdomains (see device_mgpis.hpp for the layout).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <tuple>
#include <type_traits>
#include <random>
#include <thread>

#include <rocblas/rocblas.h>
#include <rocsolver/rocsolver.h>

#include "device_mgpis.hpp"

namespace ddpca {

// ============================================================================== kernels
namespace {

enum SellMode { kSpmv = 0, kResid = 1, kJac = 2, kPcg = 3, kCheb = 4 };
enum FinWhat { kFinInit = 0, kFinBeta0 = 1, kFinAlpha = 2, kFinRR = 3, kFinBeta = 4, kFinInitWarm = 5 };

struct SellArgs {
    const int32_t* slots;
    const int64_t* off;
    const int32_t* col;
    const int16_t* col16;  // column offsets from the row node (levels whose offsets fit), or null
    const void* val;       // streamed values in the launch's ValType: double (Krylov operator), or the V-cycle
                           // copy's float / block-exponent fp16 / block-scaled int8; null in table mode
    const int32_t* csub;   // chunk -> subdomain
    int64_t nch;
    const double* x;       // gathered operand
    double* y;             // SPMV / RESID output, PCG: q (in place)
    const double* b;       // RESID / JAC / CHEB right-hand side
    const void* minv;      // smoother inverse: double, or float on reduced-precision levels
    const double* coef;    // per subdomain (c1, c2) of this sweep; JAC uses c2 = omega
    double* xo;            // JAC / CHEB new iterate
    double* p;             // PCG: p (in place), CHEB: direction d (in place)
    const PcgScal* sc;     // per-subdomain stop flags / beta; nullptr = never stopped
    double* partial;       // per chunk
    const int32_t* rtype;  // table mode: row -> table row
    const double* tab;     // table mode: tstride doubles per table row, slot-major 3x3 blocks
    int64_t tstride;
    const int32_t* ctype;  // table mode: chunk -> its rows' common table row, -1 = mixed
    // fp32 iterate copies of a block-Jacobi level (LevelDev::x4a / x4b, precond_fp32 = 4): the
    // sweep / residual gathers x (and the sweep its own row's x) from x4; the sweep writes its new
    // iterate to xo4 and / or, when xo is set (the level's last sweep), to xo in fp64
    const float4* x4;
    float4* xo4;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Chunk partial of a dot product: one wavefront = one 64-node chunk, fixed shuffle order.
__device__ __forceinline__ void chunk_partial(double v, double* partial, int64_t chunk) {
    v = wave_sum(v);
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

// Table mode: the row's blocks are the 9-double records tv[9k .. 9k+8] of its table row (shared
// with every row of the same type, so they come from L1/L2), columns prefetched one group ahead.
__device__ __forceinline__ void sell_rows_tbl(const int32_t* colp, const double* tv, const double* x, int ns,
                                              double& s0, double& s1, double& s2) {
    int k = 0;
    int32_t c0 = 0, c1 = 0, c2 = 0;
    if (ns >= 3) {
        c0 = __builtin_nontemporal_load(colp);
        c1 = __builtin_nontemporal_load(colp + kChunk);
        c2 = __builtin_nontemporal_load(colp + 2 * kChunk);
    }
    auto blk = [&](const double* v, const double* xj) {  // block_fma_any's contraction (bit-identical sums)
        const double x0 = xj[0], x1 = xj[1], x2 = xj[2];
        s0 = s0 + __builtin_fma(v[2], x2, __builtin_fma(v[1], x1, v[0] * x0));
        s1 = s1 + __builtin_fma(v[5], x2, __builtin_fma(v[4], x1, v[3] * x0));
        s2 = s2 + __builtin_fma(v[8], x2, __builtin_fma(v[7], x1, v[6] * x0));
    };
    for (; k + 3 <= ns; k += 3) {
        const int64_t j0 = c0, j1 = c1, j2 = c2;
        if (k + 6 <= ns) {
            c0 = __builtin_nontemporal_load(colp + (int64_t)(k + 3) * kChunk);
            c1 = __builtin_nontemporal_load(colp + (int64_t)(k + 4) * kChunk);
            c2 = __builtin_nontemporal_load(colp + (int64_t)(k + 5) * kChunk);
        }
        blk(tv + 9 * k, x + 3 * j0);
        blk(tv + 9 * (k + 1), x + 3 * j1);
        blk(tv + 9 * (k + 2), x + 3 * j2);
    }
    for (; k < ns; ++k) blk(tv + 9 * k, x + 3 * (int64_t)colp[(int64_t)k * kChunk]);
}

// Table mode, type-homogeneous chunk: the table row is wave-uniform, so its values are read with
// scalar loads into SGPRs (the FMAs take them as scalar operands): no per-lane value traffic.
// XV selects how x_j is read: 0 production (x stride 3, three 8-B loads); diagnostics for
// mgpis_gpu_bench_spmv: 3 x at the row's own node (coalesced bound, wrong product), 4 x stride 4
// as one 16-B + one 8-B load, 5 x stride 4 as two 16-B loads.
template <int XV = 0>
__device__ __forceinline__ void sell_rows_uniform(const int32_t* colp, const double* __restrict__ tv, const double* x,
                                                  int ns, int64_t row, double& s0, double& s1, double& s2) {
#pragma unroll 3
    for (int k = 0; k < ns; ++k) {
        const int64_t j = __builtin_nontemporal_load(colp + (int64_t)k * kChunk);
        double x0, x1, x2;
        if constexpr (XV == 3) {
            x0 = x[3 * row + (j & 0)];
            x1 = x[3 * row + 1];
            x2 = x[3 * row + 2];
        } else if constexpr (XV == 4) {
            const double2 a = reinterpret_cast<const double2*>(x)[2 * j];
            x0 = a.x;
            x1 = a.y;
            x2 = x[4 * j + 2];
        } else if constexpr (XV == 5) {
            const double2 a = reinterpret_cast<const double2*>(x)[2 * j];
            const double2 b = reinterpret_cast<const double2*>(x)[2 * j + 1];
            x0 = a.x;
            x1 = a.y;
            x2 = b.x;
        } else {
            x0 = x[3 * j];
            x1 = x[3 * j + 1];
            x2 = x[3 * j + 2];
        }
        const double* v = tv + 9 * k;
        s0 = s0 + __builtin_fma(v[2], x2, __builtin_fma(v[1], x1, v[0] * x0));
        s1 = s1 + __builtin_fma(v[5], x2, __builtin_fma(v[4], x1, v[3] * x0));
        s2 = s2 + __builtin_fma(v[8], x2, __builtin_fma(v[7], x1, v[6] * x0));
    }
}

// Production loop variant per mode.  Measured on a 1.22M-dof fine level (mgpis_gpu_bench_spmv):
// the column prefetch pays for the light-epilogue modes (y = Kx, residual), plain non-temporal
// streaming for the PCG and Chebyshev epilogues; an XCD-contiguous chunk mapping (each XCD one
// range of chunks) was 17 % slower than the dispatcher's round-robin and is gone.
constexpr int default_variant(int mode) { return (mode == 0 || mode == 1) ? 2 : 1; }

// One wavefront per 64-node chunk, one lane per node row, three accumulators per lane; T is the
// storage type of streamed operator values (all arithmetic fp64); TBL: values from the table.
template <int MODE, bool BJ, bool DOT, typename T = double, int V = default_variant(MODE), bool TBL = false,
          typename CT = int32_t, bool X4 = false>
__global__ __launch_bounds__(kBlock) void k_sell(SellArgs a, const double* __restrict__ tab) {
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    if (c >= a.nch) return;
    const int sub = a.csub[c];
    if (stopped(a.sc, sub)) return;
    const int64_t row = c * kChunk + lane;
    const int ns = a.slots[c];
    const int64_t base = a.off[c];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    if (TBL) {
        // table loop variants (mgpis_gpu_bench_spmv): 0 per-lane table rows only, 3/4/5 the
        // sell_rows_uniform diagnostics, others production
        const int ct = V == 0 ? -1 : __builtin_amdgcn_readfirstlane(a.ctype[c]);
        if (ct >= 0)
            sell_rows_uniform<(V >= 3 ? V : 0)>(a.col + base * kChunk + lane, tab + (int64_t)ct * a.tstride, a.x, ns, row,
                                                s0, s1, s2);
        else
            sell_rows_tbl(a.col + base * kChunk + lane, tab + (int64_t)a.rtype[row] * a.tstride, a.x, ns, s0, s1, s2);
    } else if constexpr (X4 && sizeof(CT) == 2)
        sell_rows<V, T, CT, float4, kGsUnroll>(a.col16 + base * kChunk + lane,
                                               static_cast<const T*>(a.val) + base * slot_vals<T>() * kChunk + lane, a.x4, ns,
                                               row, s0, s1, s2);
    else if constexpr (sizeof(CT) == 2)
        sell_rows<V, T, CT>(a.col16 + base * kChunk + lane, static_cast<const T*>(a.val) + base * slot_vals<T>() * kChunk + lane,
                            a.x, ns, row, s0, s1, s2);
    else
        sell_rows<V, T, CT>(a.col + base * kChunk + lane, static_cast<const T*>(a.val) + base * slot_vals<T>() * kChunk + lane,
                            a.x, ns, row, s0, s1, s2);
    double dotv = 0.0;
    const int64_t o = 3 * row;
    if (MODE == kSpmv) {
        a.y[o] = s0;
        a.y[o + 1] = s1;
        a.y[o + 2] = s2;
    } else if (MODE == kResid) {
        const double r0 = a.b[o] - s0, r1 = a.b[o + 1] - s1, r2 = a.b[o + 2] - s2;
        a.y[o] = r0;
        a.y[o + 1] = r1;
        a.y[o + 2] = r2;
        if (DOT) dotv = __builtin_fma(r2, r2, __builtin_fma(r1, r1, r0 * r0));
    } else if (MODE == kJac) {
        const double om = a.coef[2 * sub + 1];
        const double b0 = a.b[o], b1 = a.b[o + 1], b2 = a.b[o + 2];
        double m0, m1, m2;
        apply_m<BJ>(static_cast<const SmoothInv<T>*>(a.minv), row, b0 - s0, b1 - s1, b2 - s2, m0, m1, m2);
        // (explicit contraction throughout the epilogues: every instantiation rounds alike)
        double x0, x1, x2;
        if constexpr (X4) {
            const float4 xv = a.x4[row];
            x0 = xv.x, x1 = xv.y, x2 = xv.z;
        } else {
            x0 = a.x[o], x1 = a.x[o + 1], x2 = a.x[o + 2];
        }
        const double n0 = __builtin_fma(om, m0, x0), n1 = __builtin_fma(om, m1, x1), n2 = __builtin_fma(om, m2, x2);
        if (!X4 || a.xo) {
            a.xo[o] = n0;
            a.xo[o + 1] = n1;
            a.xo[o + 2] = n2;
        }
        if (X4 && a.xo4) a.xo4[row] = make_float4((float)n0, (float)n1, (float)n2, 0.0f);
        if (DOT) dotv = __builtin_fma(b2, n2, __builtin_fma(b1, n1, b0 * n0));
    } else if (MODE == kPcg) {
        // q = K z + beta q_old, p = z + beta p_old  (K p = K z + beta K p_old)
        const double be = a.sc[sub].beta;
        const double q0 = __builtin_fma(be, a.y[o], s0), q1 = __builtin_fma(be, a.y[o + 1], s1),
                     q2 = __builtin_fma(be, a.y[o + 2], s2);
        const double p0 = __builtin_fma(be, a.p[o], a.x[o]), p1 = __builtin_fma(be, a.p[o + 1], a.x[o + 1]),
                     p2 = __builtin_fma(be, a.p[o + 2], a.x[o + 2]);
        a.y[o] = q0;
        a.y[o + 1] = q1;
        a.y[o + 2] = q2;
        a.p[o] = p0;
        a.p[o + 1] = p1;
        a.p[o + 2] = p2;
        if (DOT) dotv = __builtin_fma(p2, q2, __builtin_fma(p1, q1, p0 * q0));
    } else if (MODE == kCheb) {
        const double c1 = a.coef[2 * sub], c2 = a.coef[2 * sub + 1];
        const double b0 = a.b[o], b1 = a.b[o + 1], b2 = a.b[o + 2];
        double m0, m1, m2;
        apply_m<BJ>(static_cast<const SmoothInv<T>*>(a.minv), row, b0 - s0, b1 - s1, b2 - s2, m0, m1, m2);
        const double d0 = __builtin_fma(c2, m0, c1 * a.p[o]), d1 = __builtin_fma(c2, m1, c1 * a.p[o + 1]),
                     d2 = __builtin_fma(c2, m2, c1 * a.p[o + 2]);
        a.p[o] = d0;
        a.p[o + 1] = d1;
        a.p[o + 2] = d2;
        const double n0 = a.x[o] + d0, n1 = a.x[o + 1] + d1, n2 = a.x[o + 2] + d2;
        a.xo[o] = n0;
        a.xo[o + 1] = n1;
        a.xo[o + 2] = n2;
        if (DOT) dotv = __builtin_fma(b2, n2, __builtin_fma(b1, n1, b0 * n0));
    }
    if (DOT) chunk_partial(dotv, a.partial, c);
}

// Small levels (fewer chunks than the chip has SIMDs): one workgroup per chunk, each of its four
// waves 16 of the chunk's rows, each lane a quarter of its row's slots (k = g, g + 4, ...), the
// quarters summed by lane shuffles -- four times the waves and a quarter of the dependent
// column -> x chain per lane.  Same operator bytes; y = Kx, residual and Jacobi-sweep epilogues
// (the V-cycle's small-level launches carry no dot product).
template <int MODE, bool BJ, typename T, typename CT, bool X4 = false>
__global__ __launch_bounds__(kBlock) void k_sell_split(SellArgs a) {
    const int64_t c = blockIdx.x;
    const int sub = a.csub[c];
    if (stopped(a.sc, sub)) return;
    const int lane = threadIdx.x & 63;
    const int rin = (threadIdx.x >> 6) * 16 + (lane & 15), g = lane >> 4;
    const int64_t row = c * kChunk + rin;
    const int ns = a.slots[c];
    const int64_t base = a.off[c];
    constexpr int64_t SV = slot_vals<T>() * kChunk;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    {
        const T* valp = static_cast<const T*>(a.val) + base * SV + rin;
        const CT* colp;
        if constexpr (sizeof(CT) == 2) colp = a.col16 + base * kChunk + rin;
        else colp = a.col + base * kChunk + rin;
#pragma unroll 2
        for (int k = g; k < ns; k += 4) {
            const int64_t j = col_of(colp[(int64_t)k * kChunk], row);
            if constexpr (X4) block_fma_any<true>(valp + (int64_t)k * SV, ldx(a.x4, j), s0, s1, s2, rin);
            else block_fma_any<true>(valp + (int64_t)k * SV, ldx(a.x, j), s0, s1, s2, rin);
        }
    }
    s0 += __shfl_xor(s0, 16, 64);
    s1 += __shfl_xor(s1, 16, 64);
    s2 += __shfl_xor(s2, 16, 64);
    s0 += __shfl_xor(s0, 32, 64);
    s1 += __shfl_xor(s1, 32, 64);
    s2 += __shfl_xor(s2, 32, 64);
    if (g != 0) return;
    const int64_t o = 3 * row;
    if (MODE == kSpmv) {
        a.y[o] = s0;
        a.y[o + 1] = s1;
        a.y[o + 2] = s2;
    } else if (MODE == kResid) {
        a.y[o] = a.b[o] - s0;
        a.y[o + 1] = a.b[o + 1] - s1;
        a.y[o + 2] = a.b[o + 2] - s2;
    } else if (MODE == kJac) {
        const double om = a.coef[2 * sub + 1];
        double m0, m1, m2;
        apply_m<BJ>(static_cast<const SmoothInv<T>*>(a.minv), row, a.b[o] - s0, a.b[o + 1] - s1, a.b[o + 2] - s2, m0, m1, m2);
        if constexpr (X4) {
            const float4 xv = a.x4[row];
            const double n0 = (double)xv.x + om * m0, n1 = (double)xv.y + om * m1, n2 = (double)xv.z + om * m2;
            if (a.xo) {
                a.xo[o] = n0;
                a.xo[o + 1] = n1;
                a.xo[o + 2] = n2;
            }
            if (a.xo4) a.xo4[row] = make_float4((float)n0, (float)n1, (float)n2, 0.0f);
        } else {
            a.xo[o] = a.x[o] + om * m0;
            a.xo[o + 1] = a.x[o + 1] + om * m1;
            a.xo[o + 2] = a.x[o + 2] + om * m2;
        }
    }
}

// Multicolour block Gauss-Seidel on the fine level (GsFine): one wavefront per colour chunk,
// lane = one row of that colour.  PH 0: forward sweep from zero over the L part, x_i = M_i (b_i -
// L_i x); PH 1: the residual after the forward sweep, r_i = -U_i x (every chunk, one launch);
// PH 2: backward sweep, x_i = M_i (b_i - L_i x - U_i x), DOT: partial = b . x_new per chunk.
// In place: rows of one colour are never each other's neighbours.
struct GsArgs {
    const int32_t* list;  // chunk ids of this launch (nullptr: chunks 0 .. n-1)
    int64_t n;
    const int32_t* rowidx;
    const int32_t* csub;
    const int32_t* nsl;
    const int32_t* nsu;
    const int64_t* offl;
    const int64_t* offu;
    const int32_t* col;
    const int16_t* col16;
    const void* val;
    const void* minv;
    double* x;
    const double* b;
    double* r;
    const PcgScal* sc;
    double* partial;
    const float* minvc;  // chunk-ordered fp32 inverses (GsFine::minvc), or null (fp64 copy): minv by row
    float4* x4;          // the fp32 iterate copy the sweeps gather (GsFine::x4), or null
    float4* r4;          // X4 residual (PH 1) in fp32 for the restriction (GsFine::r4), or null: r in fp64
    double* w;           // SSOR (k_gs_ssor): the partial sums a sweep hands to the next one, 3 per row
};

// the colour sweep's per-row tail: PH 1 stores r = -s; PH 0 / 2 store x = M (b - s) and return
// its share of b.x (DOT); ln = the row's position in its colour chunk.  X4 (GsFine::x4): the new
// x goes to the fp32 iterate copy the sweeps gather; only the backward sweep (PH 2), whose x is
// the V-cycle's output, also writes it in fp64
template <int PH, bool DOT, typename T, bool X4 = false>
__device__ __forceinline__ double gs_epilogue(const GsArgs& a, int64_t c, int ln, int64_t row, bool real, double s0,
                                              double s1, double s2) {
    const int64_t o = 3 * row;
    double dotv = 0.0;
    if (PH == 1) {
        if (real) {
            if (X4 && a.r4) {
                a.r4[row] = make_float4((float)-s0, (float)-s1, (float)-s2, 0.0f);
            } else {
                a.r[o] = -s0;
                a.r[o + 1] = -s1;
                a.r[o + 2] = -s2;
            }
        }
    } else {
        const double b0 = a.b[o], b1 = a.b[o + 1], b2 = a.b[o + 2];
        double m0, m1, m2;
        if (a.minvc) {
            const float* m = a.minvc + c * 9 * kChunk + ln;
            const double r0 = b0 - s0, r1 = b1 - s1, r2 = b2 - s2;
            // explicit contraction, as in block_fma_any (bit-identical across instantiations)
            m0 = __builtin_fma((double)m[2 * kChunk], r2, __builtin_fma((double)m[kChunk], r1, (double)m[0] * r0));
            m1 = __builtin_fma((double)m[5 * kChunk], r2, __builtin_fma((double)m[4 * kChunk], r1, (double)m[3 * kChunk] * r0));
            m2 = __builtin_fma((double)m[8 * kChunk], r2, __builtin_fma((double)m[7 * kChunk], r1, (double)m[6 * kChunk] * r0));
        } else {
            apply_m<true>(static_cast<const SmoothInv<T>*>(a.minv), row, b0 - s0, b1 - s1, b2 - s2, m0, m1, m2);
        }
        if (real) {
            if (X4) a.x4[row] = make_float4((float)m0, (float)m1, (float)m2, 0.0f);
            if (!X4 || PH == 2) {
                a.x[o] = m0;
                a.x[o + 1] = m1;
                a.x[o + 2] = m2;
            }
            if (DOT) dotv = __builtin_fma(b2, m2, __builtin_fma(b1, m1, b0 * m0));
        }
    }
    return dotv;
}

// One wave per workgroup: a colour's chunks spread over more CUs than four-wave groups (+1 % at 8
// subdomains per GPU, profiles/r03j)
template <int PH, bool DOT, typename T, typename CT, bool X4 = false>
__global__ __launch_bounds__(kWave) void k_gs(GsArgs a) {
    const int lane = threadIdx.x;
    const int64_t li = blockIdx.x;
    if (li >= a.n) return;
    const int64_t c = a.list ? (int64_t)a.list[li] : li;
    const int sub = a.csub[c];
    if (stopped(a.sc, sub)) return;
    const int32_t rr = a.rowidx[c * kChunk + lane];
    const bool real = rr >= 0;
    const int64_t row = real ? rr : ~rr;  // pad lanes gather at a real row with zero blocks
    constexpr int64_t SV = slot_vals<T>() * kChunk;
    const T* val = static_cast<const T*>(a.val);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    const CT* colp;
    if constexpr (sizeof(CT) == 2) colp = a.col16;
    else colp = a.col;
    if (PH != 1) {
        const int64_t o = a.offl[c];
        if constexpr (X4) sell_rows<1, T, CT, float4, kGsUnroll>(colp + o * kChunk + lane, val + o * SV + lane, (const float4*)a.x4, a.nsl[c], row, s0, s1, s2);
        else sell_rows<1, T, CT>(colp + o * kChunk + lane, val + o * SV + lane, (const double*)a.x, a.nsl[c], row, s0, s1, s2);
    }
    if (PH != 0) {
        const int64_t o = a.offu[c];
        if constexpr (X4) sell_rows<1, T, CT, float4, kGsUnroll>(colp + o * kChunk + lane, val + o * SV + lane, (const float4*)a.x4, a.nsu[c], row, s0, s1, s2);
        else sell_rows<1, T, CT>(colp + o * kChunk + lane, val + o * SV + lane, (const double*)a.x, a.nsu[c], row, s0, s1, s2);
    }
    const double dotv = gs_epilogue<PH, DOT, T, X4>(a, c, lane, row, real, s0, s1, s2);
    if (DOT) chunk_partial(dotv, a.partial, c);
}

// Multicolour block SSOR on the fine level (opt.smoother = 4, the reference's MULT_VCYC smoothing
// order, MGPIS.h:64-76, 101-114: a forward AND a backward sweep before and after the coarse
// correction), with the reference's reuse of the previous sweep's partial sums (its p0 / p1) so
// that each sweep reads only the blocks it must: per row the sums L x, U x of the colour split
// (L = earlier colours), w = 3 doubles per row handed from one phase to the next.
//   PH 6  forward from zero:      x = M (b - L x),          w = L x                 (L)
//   PH 7  backward:               x = M (b - w - U x)                               (U)
//   PH 8  residual:               r = w - L x   (= b - M^-1 x - L x - U x)          (L)
//   PH 9  forward from P e:       x = M (b - L x - U x),    w = b - L x             (L + U)
//   PH 10 backward:               x = M (w - U x), DOT: b . x                       (U)
// Three operator passes per V-cycle against the Gauss-Seidel pair's two.
template <int PH, bool DOT, typename T, typename CT, bool X4 = false>
__global__ __launch_bounds__(kWave) void k_gs_ssor(GsArgs a) {
    const int lane = threadIdx.x;
    const int64_t li = blockIdx.x;
    if (li >= a.n) return;
    const int64_t c = a.list ? (int64_t)a.list[li] : li;
    const int sub = a.csub[c];
    if (stopped(a.sc, sub)) return;
    const int32_t rr = a.rowidx[c * kChunk + lane];
    const bool real = rr >= 0;
    const int64_t row = real ? rr : ~rr;
    constexpr int64_t SV = slot_vals<T>() * kChunk;
    const T* val = static_cast<const T*>(a.val);
    const CT* colp;
    if constexpr (sizeof(CT) == 2) colp = a.col16;
    else colp = a.col;
    double l0 = 0.0, l1 = 0.0, l2 = 0.0, u0 = 0.0, u1 = 0.0, u2 = 0.0;
    if constexpr (PH == 6 || PH == 8 || PH == 9) {
        const int64_t o = a.offl[c];
        if constexpr (X4) sell_rows<1, T, CT>(colp + o * kChunk + lane, val + o * SV + lane, (const float4*)a.x4, a.nsl[c], row, l0, l1, l2);
        else sell_rows<1, T, CT>(colp + o * kChunk + lane, val + o * SV + lane, (const double*)a.x, a.nsl[c], row, l0, l1, l2);
    }
    if constexpr (PH == 7 || PH == 9 || PH == 10) {
        const int64_t o = a.offu[c];
        if constexpr (X4) sell_rows<1, T, CT>(colp + o * kChunk + lane, val + o * SV + lane, (const float4*)a.x4, a.nsu[c], row, u0, u1, u2);
        else sell_rows<1, T, CT>(colp + o * kChunk + lane, val + o * SV + lane, (const double*)a.x, a.nsu[c], row, u0, u1, u2);
    }
    const int64_t o = 3 * row;
    if constexpr (PH == 8) {
        if (!real) return;
        const double r0 = a.w[o] - l0, r1 = a.w[o + 1] - l1, r2 = a.w[o + 2] - l2;
        if (X4 && a.r4) {
            a.r4[row] = make_float4((float)r0, (float)r1, (float)r2, 0.0f);
        } else {
            a.r[o] = r0;
            a.r[o + 1] = r1;
            a.r[o + 2] = r2;
        }
        return;
    } else {
        const double b0 = a.b[o], b1 = a.b[o + 1], b2 = a.b[o + 2];
        double c0, c1, c2;
        if constexpr (PH == 6) {
            c0 = b0 - l0, c1 = b1 - l1, c2 = b2 - l2;
        } else if constexpr (PH == 7) {
            c0 = (b0 - a.w[o]) - u0, c1 = (b1 - a.w[o + 1]) - u1, c2 = (b2 - a.w[o + 2]) - u2;
        } else if constexpr (PH == 9) {
            c0 = (b0 - l0) - u0, c1 = (b1 - l1) - u1, c2 = (b2 - l2) - u2;
        } else {
            c0 = a.w[o] - u0, c1 = a.w[o + 1] - u1, c2 = a.w[o + 2] - u2;
        }
        const float* m = a.minvc + c * 9 * kChunk + lane;
        const double m0 = __builtin_fma((double)m[2 * kChunk], c2, __builtin_fma((double)m[kChunk], c1, (double)m[0] * c0));
        const double m1 = __builtin_fma((double)m[5 * kChunk], c2, __builtin_fma((double)m[4 * kChunk], c1, (double)m[3 * kChunk] * c0));
        const double m2 = __builtin_fma((double)m[8 * kChunk], c2, __builtin_fma((double)m[7 * kChunk], c1, (double)m[6 * kChunk] * c0));
        double dotv = 0.0;
        if (real) {
            if constexpr (PH == 6) {
                a.w[o] = l0;
                a.w[o + 1] = l1;
                a.w[o + 2] = l2;
            } else if constexpr (PH == 9) {
                a.w[o] = b0 - l0;
                a.w[o + 1] = b1 - l1;
                a.w[o + 2] = b2 - l2;
            }
            // x4 mode: every sweep writes the fp32 copy the later colours gather; the last backward
            // sweep (PH 10) also the fp64 output z
            if (X4) a.x4[row] = make_float4((float)m0, (float)m1, (float)m2, 0.0f);
            if (!X4 || PH == 10) {
                a.x[o] = m0;
                a.x[o + 1] = m1;
                a.x[o + 2] = m2;
            }
            if (DOT) dotv = __builtin_fma(b2, m2, __builtin_fma(b1, m1, b0 * m0));
        }
        if (DOT) chunk_partial(dotv, a.partial, c);
    }
}

// Band mode's rows outside the colours (GsFine::band; one wave per chunk of the ring / far groups):
// PH 5: x = 0, r = b before the forward sweep (the ring's r is recomputed by PH 3); PH 3: the
// ring's residual r = b - K x over its stored band columns (x is zero elsewhere after the forward
// sweep from zero); PH 4: the dot product's chunk partial b . x of rows the backward sweep leaves
// as the prolongation wrote them
template <int PH, typename T, typename CT>
__global__ __launch_bounds__(kWave) void k_gs_aux(GsArgs a) {
    const int lane = threadIdx.x;
    const int64_t li = blockIdx.x;
    if (li >= a.n) return;
    const int64_t c = a.list[li];
    const int sub = a.csub[c];
    if (stopped(a.sc, sub)) return;
    const int32_t rr = a.rowidx[c * kChunk + lane];
    const bool real = rr >= 0;
    const int64_t row = real ? rr : ~rr;
    const int64_t o = 3 * row;
    if (PH == 5) {
        if (real)
            for (int e = 0; e < 3; ++e) {
                a.x[o + e] = 0.0;
                a.r[o + e] = a.b[o + e];
            }
        return;
    }
    if (PH == 4) {
        const double d = real ? __builtin_fma(a.b[o + 2], a.x[o + 2], __builtin_fma(a.b[o + 1], a.x[o + 1], a.b[o] * a.x[o])) : 0.0;
        chunk_partial(d, a.partial, c);
        return;
    }
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    const CT* colp;
    if constexpr (sizeof(CT) == 2) colp = a.col16;
    else colp = a.col;
    constexpr int64_t SV = slot_vals<T>() * kChunk;
    const int64_t q = a.offl[c];
    sell_rows<1, T, CT>(colp + q * kChunk + lane, static_cast<const T*>(a.val) + q * SV + lane, (const double*)a.x, a.nsl[c], row, s0, s1, s2);
    if (real) {
        a.r[o] = a.b[o] - s0;
        a.r[o + 1] = a.b[o + 1] - s1;
        a.r[o + 2] = a.b[o + 2] - s2;
    }
}

// Node-parallel kernels: thread = node, 256 nodes per workgroup; a wavefront is one chunk, so
// the subdomain (and its stop flag) is uniform per wavefront.  nn is a multiple of 64.
#define NODE_PROLOGUE(nn, csub, sc)                         \
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; \
    if (i >= (nn)) return;                                  \
    const int sub = (csub)[i >> 6];                         \
    if (stopped((sc), sub)) return;

// x = omega M b  (first smoothing sweep from a zero guess); CHEB: also d = x
// (x4: the level's fp32 iterate copy takes x instead, LevelDev::x4a)
template <bool BJ, bool SETD, typename MT = double>
__global__ __launch_bounds__(kBlock) void k_jac0(const double* b, const MT* minv, const double* coef, double* x,
                                                 double* d, int64_t nn, const int32_t* csub, const PcgScal* sc,
                                                 float4* x4 = nullptr) {
    NODE_PROLOGUE(nn, csub, sc)
    const double om = coef[2 * sub + 1];
    double m0, m1, m2;
    apply_m<BJ>(minv, i, b[3 * i], b[3 * i + 1], b[3 * i + 2], m0, m1, m2);
    if (x4) {
        x4[i] = make_float4((float)(om * m0), (float)(om * m1), (float)(om * m2), 0.0f);
    } else {
        x[3 * i] = om * m0;
        x[3 * i + 1] = om * m1;
        x[3 * i + 2] = om * m2;
    }
    if (SETD) {
        d[3 * i] = om * m0;
        d[3 * i + 1] = om * m1;
        d[3 * i + 2] = om * m2;
    }
}

// b_c = mask_c (sum_children w r_f[child]), the coarse node's own fine copy first with w = 1;
// optionally x_c = omega M b_c (CHEB: d_c too).  Children in SELL-64 layout: slot k of chunk c
// at (roff[c] + k) * 64 + lane, so index and weight loads are contiguous wave accesses.
// 1/k for the uniform-averaging stencils (weight = 1 / number of parents; k_prolong<true>)
__constant__ double kInvCount[9] = {0.0, 1.0, 0.5, 1.0 / 3.0, 0.25, 0.2, 1.0 / 6.0, 1.0 / 7.0, 0.125};

// restriction epilogue: b_c = mask s; INIT: x_c = omega M b_c (SETD: d_c = x_c)
template <bool INIT, bool BJ, bool SETD, typename MT>
__device__ __forceinline__ void restrict_store(const uint8_t* cmask, double* bc, double* xc, double* dc, const MT* minv,
                                               const double* coef, int64_t j, int sub, double s0, double s1,
                                               double s2, float4* xc4) {
    const uint8_t m = cmask[j];
    s0 = (m & 1) ? s0 : 0.0;
    s1 = (m & 2) ? s1 : 0.0;
    s2 = (m & 4) ? s2 : 0.0;
    bc[3 * j] = s0;
    bc[3 * j + 1] = s1;
    bc[3 * j + 2] = s2;
    if (INIT) {
        const double om = coef[2 * sub + 1];
        double m0, m1, m2;
        apply_m<BJ>(minv, j, s0, s1, s2, m0, m1, m2);
        if (xc4) {  // the coarse level's fp32 iterate copy (LevelDev::x4a) instead of x_c
            xc4[j] = make_float4((float)(om * m0), (float)(om * m1), (float)(om * m2), 0.0f);
        } else {
            xc[3 * j] = om * m0;
            xc[3 * j + 1] = om * m1;
            xc[3 * j + 2] = om * m2;
        }
        if (SETD) {
            dc[3 * j] = om * m0;
            dc[3 * j + 1] = om * m1;
            dc[3 * j + 2] = om * m2;
        }
    }
}

template <bool INIT, bool BJ, bool SETD, typename MT = double>
__global__ __launch_bounds__(kBlock) void k_restrict(const double* rf, const int32_t* rslots, const int64_t* roff,
                                                     const int32_t* rcol, const double* rwt, const uint8_t* cmask,
                                                     double* bc, double* xc, double* dc, const MT* minv,
                                                     const double* coef, int64_t nc, const int32_t* csub,
                                                     const PcgScal* sc, float4* xc4) {
    NODE_PROLOGUE(nc, csub, sc)
    const int64_t j = i, c = j >> 6;
    const int ns = rslots[c];
    const int32_t* cp = rcol + roff[c] * kChunk + (j & 63);
    const double* wp = rwt + roff[c] * kChunk + (j & 63);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll 4
    for (int k = 0; k < ns; ++k) {
        const int64_t f = __builtin_nontemporal_load(cp + (int64_t)k * kChunk);
        const double w = __builtin_nontemporal_load(wp + (int64_t)k * kChunk);
        s0 += w * rf[3 * f];
        s1 += w * rf[3 * f + 1];
        s2 += w * rf[3 * f + 2];
    }
    restrict_store<INIT, BJ, SETD>(cmask, bc, xc, dc, minv, coef, j, sub, s0, s1, s2, xc4);
}

// Lattice restriction (LevelDev::lat): children f0 + d0 t0 + d1 t1 + d2 t2 for the bits of the
// coarse node's 27-bit mask, weight 2^-(|d0|+|d1|+|d2|); every index is computed, the 27 gathers
// are independent (no index / weight stream)
template <bool INIT, bool BJ, bool SETD, typename MT = double, typename RT = double>
__global__ __launch_bounds__(kBlock) void k_restrict_lat(const RT* rf, const uint32_t* rmsk, const int32_t* rf0,
                                                         const int32_t* rstr, const uint8_t* cmask, double* bc,
                                                         double* xc, double* dc, const MT* minv, const double* coef,
                                                         int64_t nc, const int32_t* csub, const PcgScal* sc,
                                                         float4* xc4) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= nc) return;
    const int sub = csub[i >> 6];
    if (stopped(sc, sub)) return;
    const int64_t j = i;
    const uint32_t msk = rmsk[j];
    const int64_t f0 = rf0[j];
    const int64_t t0 = rstr[3 * sub], t1 = rstr[3 * sub + 1], t2 = rstr[3 * sub + 2];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int q = 0; q < 27; ++q) {
        const int d0 = q % 3 - 1, d1 = (q / 3) % 3 - 1, d2 = q / 9 - 1;
        const double w = 1.0 / (double)(1 << ((d0 != 0) + (d1 != 0) + (d2 != 0)));
        const int64_t f = f0 + d0 * t0 + d1 * t1 + d2 * t2;
        if ((msk >> q) & 1u) {
            const X3 v = ldx(rf, f);  // RT = float4: the fine residual's fp32 copy (GsFine::r4), one 16-B load
            s0 += w * v.a;
            s1 += w * v.b;
            s2 += w * v.c;
        }
    }
    restrict_store<INIT, BJ, SETD>(cmask, bc, xc, dc, minv, coef, j, sub, s0, s1, s2, xc4);
}

// x_f += mask_f e into a level's fp64 iterate ...
__device__ __forceinline__ void masked_add(double* xf, int64_t i, uint8_t m, double e0, double e1, double e2) {
    if (m & 1) xf[3 * i] += e0;
    if (m & 2) xf[3 * i + 1] += e1;
    if (m & 4) xf[3 * i + 2] += e2;
}
// ... or into its fp32 iterate copy (LevelDev::x4a of a block-Jacobi level, GsFine::x4 of the
// multicolour sweeps): the add in fp64, the copy rounded once on store
__device__ __forceinline__ void masked_add(float4* x4, int64_t i, uint8_t m, double e0, double e1, double e2) {
    float4 v = x4[i];
    if (m & 1) v.x = (float)((double)v.x + e0);
    if (m & 2) v.y = (float)((double)v.y + e1);
    if (m & 4) v.z = (float)((double)v.z + e2);
    x4[i] = v;
}

// x_f += mask_f (P e_c); XT: the fine iterate (double) or its fp32 copy (float4, see masked_add),
// the sum in fp64 either way
template <bool UW = false, typename XT = double>  // UW: weights 1 / parent count (see k_restrict), pw unread
__global__ __launch_bounds__(kBlock) void k_prolong(const double* ec, const int32_t* ppar, const double* pw,
                                                    const uint8_t* fmask, XT* xf, int64_t nf, const int32_t* csub,
                                                    const PcgScal* sc) {
    NODE_PROLOGUE(nf, csub, sc)
    double e0 = 0.0, e1 = 0.0, e2 = 0.0;
    int np = 0;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        const int32_t c = ppar[p * nf + i];
        if (c < 0) break;
        const double w = UW ? 1.0 : pw[p * nf + i];
        e0 += w * ec[3 * (int64_t)c];
        e1 += w * ec[3 * (int64_t)c + 1];
        e2 += w * ec[3 * (int64_t)c + 2];
        ++np;
    }
    if (UW) {
        const double w = kInvCount[np];
        e0 *= w;
        e1 *= w;
        e2 *= w;
    }
    masked_add(xf, i, fmask[i], e0, e1, e2);
}

// Lattice prolongation (LevelDev::lat): parents p0 + the subset sums of the coarse strides the
// node's code selects, weight 1 / 2^popcount(code); one 4-B word per fine node, the (up to 8)
// parent gathers independent of each other.  XT = float4: x4_f = fp32(x4_f + mask_f 2^-k sum e_c)
// into the multicolour sweeps' copy (what the backward sweep then gathers) or a block-Jacobi level's
template <typename XT = double>
__global__ __launch_bounds__(kBlock) void k_prolong_lat(const double* ec, const uint32_t* ppk, const int32_t* pstr,
                                                        const uint8_t* fmask, XT* xf, int64_t nf,
                                                        const int32_t* csub, const PcgScal* sc) {
    NODE_PROLOGUE(nf, csub, sc)
    const uint32_t w = ppk[i];
    const int64_t p0 = w & 0x1fffffffu;
    const uint32_t code = w >> 29;
    const int64_t s0 = pstr[3 * sub], s1 = pstr[3 * sub + 1], s2 = pstr[3 * sub + 2];
    double e0 = 0.0, e1 = 0.0, e2 = 0.0;
    // every lane issues all eight parent loads (a parent outside the node's subset reads p0 and
    // weighs 0): no divergent branches, the loads issue back to back (47.8 -> 46.0 us per fine
    // launch against the branching form, profiles/r02m_prolong_ab.txt)
#pragma unroll
    for (uint32_t q = 0; q < 8; ++q) {
        const bool in = (q & ~code) == 0;
        const int64_t c = in ? p0 + ((q & 1) ? s0 : 0) + ((q & 2) ? s1 : 0) + ((q & 4) ? s2 : 0) : p0;
        const double w = in ? 1.0 : 0.0;
        e0 += w * ec[3 * c];
        e1 += w * ec[3 * c + 1];
        e2 += w * ec[3 * c + 2];
    }
    const double wt = 1.0 / (double)(1 << __popc(code));
    masked_add(xf, i, fmask[i], wt * e0, wt * e1, wt * e2);
}

// Block transfer entries (rotated nodes): x_f += mask_f (B e_c) per fine node that owns one
// (after k_prolong, whose weight for those entries is 0); thread = fine node.  XT as in k_prolong
template <typename XT = double>
__global__ __launch_bounds__(kBlock) void k_prolong_rot(const double* ec, const int32_t* row, const int64_t* ptr,
                                                        const int32_t* par, const double* blk, const uint8_t* fmask,
                                                        XT* xf, int64_t nr, const int32_t* csub,
                                                        const PcgScal* sc) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= nr) return;
    const int64_t i = row[t];
    if (stopped(sc, csub[i >> 6])) return;
    double e0 = 0.0, e1 = 0.0, e2 = 0.0;
    for (int64_t k = ptr[t]; k < ptr[t + 1]; ++k) {
        const double* B = blk + 9 * k;
        const int64_t c = par[k];
        const double c0 = ec[3 * c], c1 = ec[3 * c + 1], c2 = ec[3 * c + 2];
        e0 += B[0] * c0 + B[1] * c1 + B[2] * c2;
        e1 += B[3] * c0 + B[4] * c1 + B[5] * c2;
        e2 += B[6] * c0 + B[7] * c1 + B[8] * c2;
    }
    masked_add(xf, i, fmask[i], e0, e1, e2);
}

// ... and b_c += mask_c (B^T r_f) per coarse node that receives one (after k_restrict).
__global__ __launch_bounds__(kBlock) void k_restrict_rot(const double* rf, const int32_t* row, const int64_t* ptr,
                                                         const int32_t* kid, const double* blk, const uint8_t* cmask,
                                                         double* bc, int64_t nr, const int32_t* csub,
                                                         const PcgScal* sc) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= nr) return;
    const int64_t j = row[t];
    if (stopped(sc, csub[j >> 6])) return;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int64_t k = ptr[t]; k < ptr[t + 1]; ++k) {
        const double* B = blk + 9 * k;
        const int64_t f = kid[k];
        const double r0 = rf[3 * f], r1 = rf[3 * f + 1], r2 = rf[3 * f + 2];
        s0 += B[0] * r0 + B[3] * r1 + B[6] * r2;
        s1 += B[1] * r0 + B[4] * r1 + B[7] * r2;
        s2 += B[2] * r0 + B[5] * r1 + B[8] * r2;
    }
    const uint8_t m = cmask[j];
    if (m & 1) bc[3 * j] += s0;
    if (m & 2) bc[3 * j + 1] += s1;
    if (m & 4) bc[3 * j + 2] += s2;
}

// x0 = A0^-1 b0 per subdomain, one wavefront per coarse dof row.  Rows are padded to a multiple of
// 4 entries (ld, zero-filled), so every lane loads 16 B of the inverse per instruction (four fp32
// or two fp64 entries) and the matching b entries as fp64 pairs; two such loads in flight per lane.
// The padding reads b of the member's padding nodes, which the masked restriction keeps at zero.
template <typename AT = double>
__global__ __launch_bounds__(kBlock) void k_coarse(const AT* ainv, const int64_t* aoff, const int64_t* noff,
                                                   const int64_t* n0, const int64_t* ldv, const double* b, double* x,
                                                   int64_t nrow, const int32_t* csub, const PcgScal* sc) {
    const int64_t r = (int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    if (r >= nrow) return;
    const int sub = csub[(r / 3) >> 6];
    if (stopped(sc, sub)) return;
    const int lane = threadIdx.x & 63;
    const int64_t lr = r - 3 * noff[sub], n = n0[sub], ld = ldv[sub];
    if (lr >= n) {
        if (lane == 0) x[r] = 0.0;
        return;
    }
    const AT* arow = ainv + aoff[sub] + lr * ld;
    const double* bs = b + 3 * noff[sub];
    constexpr int V = 16 / sizeof(AT);  // entries per 16-B load
    double s0 = 0.0, s1 = 0.0;
    auto chunk = [&](int64_t k) {
        double acc = 0.0;
        if constexpr (V == 4) {
            const float4 a = *reinterpret_cast<const float4*>(arow + k);
            const double2 b0 = *reinterpret_cast<const double2*>(bs + k), b1 = *reinterpret_cast<const double2*>(bs + k + 2);
            acc = (double)a.x * b0.x + (double)a.y * b0.y + (double)a.z * b1.x + (double)a.w * b1.y;
        } else {
            const double2 a = *reinterpret_cast<const double2*>(arow + k);
            const double2 b0 = *reinterpret_cast<const double2*>(bs + k);
            acc = a.x * b0.x + a.y * b0.y;
        }
        return acc;
    };
    int64_t k = (int64_t)V * lane;
    for (; k + V * kWave < ld; k += 2 * V * kWave) {
        s0 += chunk(k);
        s1 += chunk(k + V * kWave);
    }
    if (k < ld) s0 += chunk(k);
    const double s = wave_sum(s0 + s1);
    if (lane == 0) x[r] = s;
}

// r = b, x = p = q = 0, partial ||b||^2 per chunk
__global__ __launch_bounds__(kBlock) void k_pcg_init(const double* b, double* x, double* r, double* p, double* q,
                                                     double* partial, int64_t nn) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= nn) return;
    double s = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double v = b[3 * i + a];
        r[3 * i + a] = v;
        x[3 * i + a] = 0.0;
        p[3 * i + a] = 0.0;
        q[3 * i + a] = 0.0;
        s += v * v;
    }
    chunk_partial(s, partial, i >> 6);
}

// warm start: p = q = 0, partial ||b||^2 per chunk (r = b - K x0 by k_sell<kResid>)
__global__ __launch_bounds__(kBlock) void k_pcg_init_warm(const double* b, double* p, double* q, double* partial,
                                                          int64_t nn) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= nn) return;
    double s = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double v = b[3 * i + a];
        p[3 * i + a] = 0.0;
        q[3 * i + a] = 0.0;
        s += v * v;
    }
    chunk_partial(s, partial, i >> 6);
}

// x += alpha p, r -= alpha q, partial ||r||^2
// x += alpha p, r -= alpha q, partial ||r||^2.  One wavefront per 64-node chunk walks the chunk's
// 192 doubles flat (lane, lane + 64, lane + 128): every load is a contiguous 512-B wave access
// instead of three 24-B-strided ones.
__global__ __launch_bounds__(kBlock) void k_axpy(double* x, double* r, const double* p, const double* q,
                                                 const PcgScal* sc, double* partial, int64_t nn, const int32_t* csub) {
    const int64_t c = (int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    if (c * kChunk >= nn) return;
    const int sub = csub[c];
    if (stopped(sc, sub)) return;
    const double al = sc[sub].alpha;
    const int64_t base = c * 3 * kChunk + (threadIdx.x & 63);
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int64_t k = base + j * kChunk;
        x[k] += al * p[k];
        const double v = r[k] - al * q[k];
        r[k] = v;
        s += v * v;
    }
    chunk_partial(s, partial, c);
}

// z = D^-1 r (diagonal preconditioner, DIAG_PREC), partial r^T z
__global__ __launch_bounds__(kBlock) void k_diag(const double* r, const double* dinv, double* z, double* partial,
                                                 int64_t nn, const int32_t* csub, const PcgScal* sc) {
    NODE_PROLOGUE(nn, csub, sc)
    double s = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double v = dinv[3 * i + a] * r[3 * i + a];
        z[3 * i + a] = v;
        s += r[3 * i + a] * v;
    }
    chunk_partial(s, partial, i >> 6);
}

// partial x^T y per chunk (used after a coarse-only "V-cycle")
__global__ __launch_bounds__(kBlock) void k_dot(const double* x, const double* y, double* partial, int64_t nn,
                                                const int32_t* csub, const PcgScal* sc) {
    NODE_PROLOGUE(nn, csub, sc)
    double s = 0.0;
    for (int a = 0; a < 3; ++a) s += x[3 * i + a] * y[3 * i + a];
    chunk_partial(s, partial, i >> 6);
}

// Scalar updates of the PCG recurrence: one workgroup per subdomain, fixed summation order
// over that subdomain's chunk partials.  Stop-state changes are mirrored to host memory.
// kFinT = 1024 threads read a subdomain's ~6400 fine chunk partials in ~2 loads each (256: 0.2-0.6 %
// slower overall, profiles/r02u_ab.json)
constexpr int kFinT = 1024;
__global__ __launch_bounds__(kFinT) void k_fin(int what, const double* partial, const double* partial2,
                                               const int64_t* cb, PcgScal* scv, PcgMirror* mirror) {
    const int sub = blockIdx.x;
    PcgScal* sc = scv + sub;
    if (what != kFinInit && what != kFinInitWarm && sc->done) return;
    __shared__ double red[kFinT / kWave], red2[kFinT / kWave];
    // four independent accumulators per thread (loads in flight together), fixed combine order
    double a[4] = {0.0, 0.0, 0.0, 0.0}, b[4] = {0.0, 0.0, 0.0, 0.0};
    const int64_t k0 = cb[sub], k1 = cb[sub + 1];
    for (int64_t k = k0 + threadIdx.x; k < k1; k += 4 * kFinT) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t q = k + (int64_t)u * kFinT;
            if (q < k1) {
                a[u] += partial[q];
                if (what == kFinInitWarm) b[u] += partial2[q];
            }
        }
    }
    double s = wave_sum((a[0] + a[1]) + (a[2] + a[3]));
    double s2 = wave_sum((b[0] + b[1]) + (b[2] + b[3]));
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = s;
        red2[threadIdx.x >> 6] = s2;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    s = 0.0;
    s2 = 0.0;
    for (int w = 0; w < kFinT / kWave; w += 4) {
        s += (red[w] + red[w + 1]) + (red[w + 2] + red[w + 3]);
        s2 += (red2[w] + red2[w + 1]) + (red2[w + 2] + red2[w + 3]);
    }
    const int was_done = sc->done;
    if (what == kFinInit || what == kFinInitWarm) {
        const double bb = what == kFinInit ? s : s2;
        sc->rr = s;
        sc->bb = bb;
        sc->tol2 = sc->tol2 * bb;  // tol2 holds rtol^2 on entry
        sc->iter = 0;
        sc->fail = 0;
        sc->beta = 0.0;
        sc->done = (s <= sc->tol2 || sc->maxit <= 0) ? 1 : 0;
        mirror_store(mirror + sub, 0, sc->done, 0);
        return;
    } else if (what == kFinBeta0) {
        sc->delta = s;
        sc->beta = 0.0;
    } else if (what == kFinAlpha) {
        sc->pq = s;
        if (!(s > 0.0) || !isfinite(s)) {
            sc->fail = 1;
            sc->done = 1;
        }
        sc->alpha = sc->delta / s;
    } else if (what == kFinRR) {
        sc->rr = s;
        sc->iter += 1;
        if (!isfinite(s)) {
            sc->fail = 1;
            sc->done = 1;
        }
        if (s <= sc->tol2 || sc->iter >= sc->maxit) sc->done = 1;
        mirror_store(mirror + sub, sc->iter, sc->done, sc->fail);
        return;
    } else {
        if (!isfinite(s)) {
            sc->fail = 1;
            sc->done = 1;
        }
        sc->beta = s / sc->delta;
        sc->delta = s;
    }
    if (sc->done != was_done) mirror_store(mirror + sub, sc->iter, sc->done, sc->fail);
}

// full[free_dof[i]] = cond[i] (full zero-filled first) / cond[i] = full[free_dof[i]]
__global__ void k_scatter(const double* cond, const int32_t* free_dof, double* full, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) full[free_dof[i]] = cond[i];
}
__global__ void k_gather(const double* full, const int32_t* free_dof, double* cond, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) cond[i] = full[free_dof[i]];
}

// y = M x, partial ||y||^2 per chunk (power iteration for lambda_max(M K) at setup)
template <bool BJ, typename MT = double>
__global__ void k_apply_m(const double* x, const MT* minv, double* y, double* partial, int64_t nn) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= nn) return;
    double m0, m1, m2;
    apply_m<BJ>(minv, i, x[3 * i], x[3 * i + 1], x[3 * i + 2], m0, m1, m2);
    y[3 * i] = m0;
    y[3 * i + 1] = m1;
    y[3 * i + 2] = m2;
    chunk_partial(m0 * m0 + m1 * m1 + m2 * m2, partial, i >> 6);
}

// v = w * scale[subdomain]
__global__ void k_scale_sub(const double* w, const double* scale, double* v, int64_t nn, const int32_t* csub) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= nn) return;
    const double s = scale[csub[i >> 6]];
    for (int a = 0; a < 3; ++a) v[3 * i + a] = w[3 * i + a] * s;
}

// ---- host helpers
__global__ void k_mirror_upper(double* A, int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * n) return;
    const int64_t i = idx / n, j = idx % n;
    if (j < i) A[i * n + j] = A[j * n + i];
}

// In-place inverse of a dense SPD matrix (row-major = column-major, it is symmetric) with
// rocSOLVER potrf + potri on the device (setup only).
void invert_spd_device(std::vector<double>& A, int64_t n, hipStream_t st) {
    DevBuf<double> d;
    d.upload(A);
    DevBuf<rocblas_int> info(2);
    info.zero(st);
    auto solver_guard = solver_lock();
    rocblas_handle h = nullptr;
    if (rocblas_create_handle(&h) != rocblas_status_success) throw ApiError(DDPCA_EHIP, "rocblas_create_handle");
    rocblas_set_stream(h, st);
    const rocblas_status s1 = rocsolver_dpotrf(h, rocblas_fill_lower, (rocblas_int)n, d.p, (rocblas_int)n, info.p);
    const rocblas_status s2 = rocsolver_dpotri(h, rocblas_fill_lower, (rocblas_int)n, d.p, (rocblas_int)n, info.p + 1);
    hipLaunchKernelGGL(k_mirror_upper, dim3(std::max<int64_t>(1, (n * n + 255) / 256)), dim3(256), 0, st, d.p, n);
    DDPCA_HIP(hipStreamSynchronize(st));
    rocblas_destroy_handle(h);
    const auto inf = info.download();
    if (s1 != rocblas_status_success || s2 != rocblas_status_success) throw ApiError(DDPCA_EHIP, "rocsolver potrf/potri failed");
    if (inf[0] != 0 || inf[1] != 0) throw ApiError(DDPCA_ENUMERIC, "coarse operator is not positive definite");
    DDPCA_HIP(hipMemcpy(A.data(), d.p, A.size() * sizeof(double), hipMemcpyDeviceToHost));
}

// Scale row i of the column-major n x n matrix Vt by 1 / s_i, or 0 when s_i <= tol (pseudo-inverse)
__global__ void k_pinv_rows(double* Vt, const double* S, int64_t n, double tol) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * n) return;
    const double sv = S[idx % n];
    Vt[idx] *= sv > tol ? 1.0 / sv : 0.0;
}

__global__ void k_diag(const double* A, int64_t n, double* d) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) d[i] = A[i * n + i];
}

// row sums of |M - I| (M column-major n x n): the residual of an inverse read as M = A^-1 A
__global__ void k_resid_rows(const double* M, int64_t n, double* r) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) s += std::abs(M[i * n + j] - (i == j ? 1.0 : 0.0));
    r[j] = s;
}

// In-place inverse of a dense general matrix by rocSOLVER getrf + getri when its LU is clearly
// regular (every |U_ii| above 1e-10 of the largest) and the inverse checks out (||A^-1 A - I||_inf
// <= kLuMaxResid by a rocBLAS gemm against the kept copy of A); returns false, A untouched,
// otherwise, and *resid the residual it measured (INFINITY when the pivot test failed).  The
// column-major view of the row-major buffer is A^T, whose inverse read back row-major is A^-1.
// (LAGRANGE's condensed coarse operators, 4851 rows at BLOCK: ~20 s per Newton step by gesvd.)
constexpr double kLuMaxResid = 1e-6;
bool inv_general_lu_device(std::vector<double>& A, int64_t n, hipStream_t st, double* resid) {
    *resid = INFINITY;
    DevBuf<double> d, a0, diag(std::max<int64_t>(n, 1));
    d.upload(A);
    a0.upload(A);
    DevBuf<rocblas_int> ipiv(std::max<int64_t>(n, 1)), info(2);
    info.zero(st);
    auto solver_guard = solver_lock();
    rocblas_handle h = nullptr;
    if (rocblas_create_handle(&h) != rocblas_status_success) throw ApiError(DDPCA_EHIP, "rocblas_create_handle");
    rocblas_set_stream(h, st);
    const rocblas_status s1 = rocsolver_dgetrf(h, (rocblas_int)n, (rocblas_int)n, d.p, (rocblas_int)n, ipiv.p, info.p);
    hipLaunchKernelGGL(k_diag, dim3(std::max<int64_t>(1, (n + 255) / 256)), dim3(256), 0, st, d.p, n, diag.p);
    DDPCA_HIP(hipStreamSynchronize(st));
    const auto u = diag.download();
    double umax = 0.0, umin = INFINITY;
    for (double x : u) {
        umax = std::max(umax, std::abs(x));
        umin = std::min(umin, std::abs(x));
    }
    if (s1 != rocblas_status_success || info.download()[0] != 0 || !(umin > 1e-10 * umax)) {
        rocblas_destroy_handle(h);
        return false;
    }
    const rocblas_status s2 = rocsolver_dgetri(h, (rocblas_int)n, d.p, (rocblas_int)n, ipiv.p, info.p + 1);
    // column-major: d = (A^T)^-1 and a0 = A^T, so M = d a0 = (A A^-1)^T; ||M - I|| by column sums
    // of M (= row sums of A A^-1 - I)
    DevBuf<double> M(std::max<int64_t>(n * n, 1)), rs(std::max<int64_t>(n, 1));
    const double one = 1.0, zero = 0.0;
    const rocblas_status s3 = rocblas_dgemm(h, rocblas_operation_none, rocblas_operation_none, (rocblas_int)n, (rocblas_int)n,
                                            (rocblas_int)n, &one, d.p, (rocblas_int)n, a0.p, (rocblas_int)n, &zero, M.p,
                                            (rocblas_int)n);
    hipLaunchKernelGGL(k_resid_rows, dim3(std::max<int64_t>(1, (n + 255) / 256)), dim3(256), 0, st, M.p, n, rs.p);
    DDPCA_HIP(hipStreamSynchronize(st));
    rocblas_destroy_handle(h);
    if (s2 != rocblas_status_success || s3 != rocblas_status_success || info.download()[1] != 0) return false;
    double r = 0.0;
    for (double x : rs.download()) r = std::max(r, x);
    *resid = r;
    if (!(r <= kLuMaxResid)) return false;
    DDPCA_HIP(hipMemcpy(A.data(), d.p, A.size() * sizeof(double), hipMemcpyDeviceToHost));
    return true;
}

// In-place pseudo-inverse of a dense general matrix (setup only): rocSOLVER gesvd of the buffer
// read column-major (M = A^T = U S Vt), then C = Vt^T S+ U^T (rocBLAS gemm) = (A^+)^T column-major,
// i.e. A^+ row-major.  Singular values below 1e-11 of the largest are dropped: the coarse operator
// of LAGRANGE's condensed system is singular when a frictionless contact leaves a body free to
// slide (the reference's LDLT meets the same zero pivots); the V-cycle then solves on the range.
void pinv_general_device(std::vector<double>& A, int64_t n, hipStream_t st, int64_t* dropped) {
    DevBuf<double> d, S(std::max<int64_t>(n, 1)), U(std::max<int64_t>(n * n, 1)), Vt(std::max<int64_t>(n * n, 1)),
        E(std::max<int64_t>(n, 1)), C(std::max<int64_t>(n * n, 1));
    d.upload(A);
    DevBuf<rocblas_int> info(1);
    info.zero(st);
    auto solver_guard = solver_lock();
    rocblas_handle h = nullptr;
    if (rocblas_create_handle(&h) != rocblas_status_success) throw ApiError(DDPCA_EHIP, "rocblas_create_handle");
    rocblas_set_stream(h, st);
    const rocblas_status s1 = rocsolver_dgesvd(h, rocblas_svect_all, rocblas_svect_all, (rocblas_int)n, (rocblas_int)n, d.p,
                                               (rocblas_int)n, S.p, U.p, (rocblas_int)n, Vt.p, (rocblas_int)n, E.p,
                                               rocblas_outofplace, info.p);
    std::vector<double> sv(n);
    DDPCA_HIP(hipMemcpyAsync(sv.data(), S.p, n * sizeof(double), hipMemcpyDeviceToHost, st));
    DDPCA_HIP(hipStreamSynchronize(st));
    const auto inf = info.download();
    if (s1 != rocblas_status_success || inf[0] != 0) {
        rocblas_destroy_handle(h);
        throw ApiError(DDPCA_EHIP, "rocsolver gesvd failed on the coarse operator");
    }
    const double tol = 1e-11 * (n ? sv[0] : 0.0);
    *dropped = 0;
    for (double x : sv) *dropped += !(x > tol);
    hipLaunchKernelGGL(k_pinv_rows, dim3(std::max<int64_t>(1, (n * n + 255) / 256)), dim3(256), 0, st, Vt.p, S.p, n, tol);
    const double one = 1.0, zero = 0.0;
    const rocblas_status s2 = rocblas_dgemm(h, rocblas_operation_transpose, rocblas_operation_transpose, (rocblas_int)n,
                                            (rocblas_int)n, (rocblas_int)n, &one, Vt.p, (rocblas_int)n, U.p, (rocblas_int)n,
                                            &zero, C.p, (rocblas_int)n);
    DDPCA_HIP(hipStreamSynchronize(st));
    rocblas_destroy_handle(h);
    if (s2 != rocblas_status_success) throw ApiError(DDPCA_EHIP, "rocblas gemm failed");
    DDPCA_HIP(hipMemcpy(A.data(), C.p, A.size() * sizeof(double), hipMemcpyDeviceToHost));
}

}  // namespace

// ============================================================================== host plumbing
void select_device(int device) {
    static thread_local int checked = -1;  // last device verified to be a gfx950 part
    if (device == checked) {
        DDPCA_HIP(hipSetDevice(device));
        return;
    }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) throw ApiError(DDPCA_ENOGPU, "no HIP device visible");
    if (device < 0 || device >= n) throw ApiError(DDPCA_EINVAL, "device index out of range");
    DDPCA_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    DDPCA_HIP(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        throw ApiError(DDPCA_ENOGPU, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950");
    checked = device;
}

void MirrorBuf::alloc(int count) {
    n = count;
    DDPCA_HIP(hipHostMalloc(reinterpret_cast<void**>(&host), std::max(1, count) * sizeof(PcgMirror),
                            hipHostMallocMapped | hipHostMallocCoherent));
    DDPCA_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&dev), host, 0));
    reset();
}

void MirrorBuf::reset() { std::memset(host, 0, std::max(1, n) * sizeof(PcgMirror)); }

MirrorBuf::~MirrorBuf() {
    if (host) (void)hipHostFree(host);
}

int64_t pace_until_done(hipStream_t stream, hipGraphExec_t graph, const MirrorBuf& m, int64_t k, int64_t launched,
                        hipGraphExec_t graph1, int64_t horizon) {
    constexpr int64_t kRunway = 2;  // tail: single iterations kept this far ahead of the slowest member
    int64_t replays = 0;
    for (int64_t spin = 0;; ++spin) {
        bool all = true;
        int64_t slowest = INT64_MAX;
        for (int s = 0; s < m.n; ++s) {
            if (__atomic_load_n(&m.host[s].done, __ATOMIC_ACQUIRE)) continue;
            all = false;
            slowest = std::min<int64_t>(slowest, __atomic_load_n(&m.host[s].iter, __ATOMIC_RELAXED));
        }
        if (all) return replays;
        // keep one replay of runway: launch when the slowest solve has entered the last one;
        // past the expected iteration count, single iterations kRunway ahead
        const bool tail = graph1 && launched + k > horizon;
        if (tail ? launched - slowest <= kRunway : launched - slowest <= k) {
            DDPCA_HIP(hipGraphLaunch(tail ? graph1 : graph, stream));
            launched += tail ? 1 : k;
            ++replays;
            continue;
        }
        if ((spin & 255) == 255) {
            const hipError_t q = hipStreamQuery(stream);
            if (q == hipSuccess) {
                // stream drained: the mirror is final for everything enqueued so far
                bool done_now = true;
                for (int s = 0; s < m.n; ++s) done_now &= __atomic_load_n(&m.host[s].done, __ATOMIC_ACQUIRE) != 0;
                if (done_now) return replays;
                DDPCA_HIP(hipGraphLaunch(tail ? graph1 : graph, stream));
                launched += tail ? 1 : k;
                ++replays;
            } else if (q != hipErrorNotReady) {
                DDPCA_HIP(q);
            }
        }
        std::this_thread::yield();
    }
}

// ============================================================================== setup
// What reaches the device is planned on the host in mgpis_plan.cpp; here a plan is uploaded,
// array by array, and dropped.
namespace {
// the one array of V into the buffer of its storage type
void upload_values(const BlockValues& V, DevBuf<double>& d64, DevBuf<float>& d32, DevBuf<uint16_t>& d16, DevBuf<uint8_t>& d8) {
    if (V.vt == kValQ8) d8.upload(V.v8);
    else if (V.vt == kValH16) d16.upload(V.v16);
    else if (V.vt == kVal32) d32.upload(V.v32);
    else d64.upload(V.v64.get(), V.n);
}

// shape, SELL index arrays and table of a level (its values follow, copy by copy)
void upload_index(LevelDev& L, const LevelPlan& P) {
    static_cast<LevelShape&>(L) = P;
    L.slots.upload(P.slots);
    L.csub.upload(P.csub);
    L.off.upload(P.off);
    L.col.upload(P.col);
    if (!P.col16.empty()) L.col16.upload(P.col16);
    if (P.tbl) {
        L.rtype.upload(P.rtype);
        L.ctype.upload(P.ctype);
        L.tab.upload(P.tab);
    }
}

void upload_colours(GsFine& G, const ColourPlan& P) {
    static_cast<ColourShape&>(G) = P;
    if (!P.minvc.empty()) G.minvc.upload(P.minvc);
    G.list.upload(P.list);
    G.rowidx.upload(P.rowidx);
    G.csub.upload(P.csub);
    G.nsl.upload(P.nsl);
    G.nsu.upload(P.nsu);
    G.offl.upload(P.offl);
    G.offu.upload(P.offu);
    G.cb.upload(P.cb);
    if (!P.col16.empty()) G.col16.upload(P.col16);
    else G.col.upload(P.col);
    upload_values(P.val, G.val64, G.val32, G.val16, G.val8);
}

void upload_transfer(LevelDev& L, const TransferPlan& T) {
    static_cast<TransferShape&>(L) = T;
    if (T.nrot) {
        L.rot_row.upload(T.rot_row);
        L.rot_ptr.upload(T.rot_ptr);
        L.rot_par.upload(T.rot_par);
        L.rot_blk.upload(T.rot_blk);
        L.rotc_row.upload(T.rotc_row);
        L.rotc_ptr.upload(T.rotc_ptr);
        L.rotc_kid.upload(T.rotc_kid);
        L.rotc_blk.upload(T.rotc_blk);
    }
    if (T.lat) {
        L.ppk.upload(T.ppk);
        L.pstr.upload(T.pstr);
        L.rmsk.upload(T.rmsk);
        L.rf0.upload(T.rf0);
        L.rstr.upload(T.rstr);
        return;
    }
    L.ppar.upload(T.ppar);
    if (!T.uw) L.pw.upload(T.pw);
    L.rslots.upload(T.rslots);
    L.roff.upload(T.roff);
    L.rcol.upload(T.rcol);
    L.rwt.upload(T.rwt);
}
}  // namespace

MgpisDevice::MgpisDevice(int dev, const std::vector<SubdomainOps>& subs, const mgpis_options_t& o, bool gen,
                         bool diag_only)
    : general(gen), device(dev), opt(o) {
    // ---- validate
    select_device(device);
    nsub = (int)subs.size();
    if (nsub < 1) throw ApiError(DDPCA_EINVAL, "empty subdomain batch");
    const int nlev = (int)subs[0].nnodes.size();
    for (const auto& S : subs) {
        if ((int)S.nnodes.size() != nlev || nlev < 1 || (int)S.K.size() != nlev || (int)S.S.size() != nlev - 1)
            throw ApiError(DDPCA_EINVAL, "level counts differ within the batch");
        if (!S.dof_free) throw ApiError(DDPCA_EINVAL, "dof_free missing");
        for (int l = 0; l < nlev; ++l)
            if (S.K[l]->nb != S.nnodes[l] || S.K[l]->mb != S.nnodes[l]) throw ApiError(DDPCA_EINVAL, "operator size does not match nnodes");
    }
    DDPCA_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    if (opt.nu < 1) opt.nu = 1;
    if (opt.iters_per_graph < 1) opt.iters_per_graph = 1;
    if (opt.smoother < 0 || opt.smoother > 4) throw ApiError(DDPCA_EINVAL, "smoother must be 0..4");
    // the multicolour sweeps' symmetric pairing needs K = K^T: nonsymmetric handles smooth with block Jacobi
    if (opt.smoother >= 3 && general) opt.smoother = 1;
    // (refused here, not at the first capture's launch_gs; one level has no V-cycle and no
    // colours: the option is idle there, as smoother 3 is)
    if (opt.smoother == 4 && opt.precond_fp32 == 0 && nlev > 1)
        throw ApiError(DDPCA_ESTATE, "colour SSOR needs a reduced-precision V-cycle copy (precond_fp32 >= 1)");
    const bool bj = opt.smoother >= 1;
    const MgpisTuning tune = mgpis_tuning();  // the create-time variables, read once per handle

    // ---- number the nodes
    MgpisNumbering num = mgpis_numbering(subs, opt.table_mode);

    // ---- per level: plan, upload, drop the plan
    lev.resize(nlev);
    for (int l = 0; l < nlev; ++l) {
        LevelDev& L = lev[l];
        {
            LevelPlan P = plan_level(subs, num, l, bj, opt.table_mode, tune);
            upload_index(L, P);
            std::vector<int16_t>().swap(P.col16);  // (a quarter of the index arrays: not held while the values are packed)
            // fp64 values: the fine level (Krylov operator) and, without the reduced-precision
            // preconditioner copy, every level; the copy serves the V-cycle on levels >= 1 (level 0
            // is the dense inverse).  Table-mode levels need neither.
            const bool copy = !P.tbl && vc32() && l >= 1;
            if (!P.tbl && (l == nlev - 1 || !vc32())) upload_values(pack_values(P, kVal64), L.val, L.val32, L.val16, L.val8);
            if (copy)
                upload_values(level_copy(P, level_copy_type(opt.precond_fp32, l, nlev, tune), l, tune), L.val, L.val32, L.val16,
                              L.val8);
            L.dinv.upload(P.dinv);
            L.minv.upload(P.minv);
            // reduced-precision levels smooth with an fp32 inverse
            std::vector<float> m32;
            if (copy) {
                m32 = smoother_inverse_fp32(P.minv, bj, !general);
                L.minv32.upload(m32);
            }
            if (l == nlev - 1 && nlev > 1 && opt.smoother >= 3) {
                // band mode (locally refined fine level): elsewhere the stencils are level
                // l - 1's, which the V-cycle smooths next (colour SSOR sweeps every row)
                std::vector<uint8_t> band;
                if (opt.smoother == 3) band = colour_band(subs, num, l, P, tune);
                upload_colours(gs, plan_colours(P, vc_type(l), copy ? &m32 : nullptr, band.empty() ? nullptr : &band, tune));
            }
            L.mask.upload(P.mask);
        }
        for (auto* v : {&L.x, &L.t, &L.b, &L.r, &L.d}) {
            v->alloc(3 * L.nn);
            v->zero(stream);
        }
        if (l > 0) upload_transfer(L, plan_transfer(subs, num, l, L, lev[l - 1], tune));
    }
    level_perm = std::move(num.perm);
    fine_perm = level_perm[nlev - 1];

    // ---- exact coarse solve: dense inverse of each subdomain's masked operator on level clev, in
    // that level's device order.  A one-level handle too large for a dense inverse serves the
    // diagonal-preconditioned drivers only (precSwit 0; the V-cycle then reports DDPCA_ESTATE)
    int64_t n0max = 0;
    clev = choose_coarse_level(subs, opt.coarse_level, &n0max);
    no_coarse = diag_only || (nlev == 1 && n0max > 12288);
    if (!no_coarse) {
        std::vector<double> packed;
        std::vector<int64_t> ao(nsub), no(nsub), nz(nsub), ldv(nsub);
        for (int s = 0; s < nsub; ++s) {
            const auto& p = level_perm[clev][s];
            const int64_t n0 = 3 * subs[s].nnodes[clev];
            std::vector<double> D = coarse_dense(subs[s], clev, p, general);
            if (general) {
                // LU inverse when the LU is clearly regular, else the SVD pseudo-inverse
                double resid = INFINITY;
                const bool lu = inv_general_lu_device(D, n0, stream, &resid);
                int64_t dropped = 0;
                if (!lu) pinv_general_device(D, n0, stream, &dropped);
                coarse_inverse.push_back({lu ? 1 : 2, resid, dropped});
                if (tune.verbose)
                    std::fprintf(stderr, "[ddpca] coarse inverse: %s, %ld rows, LU residual %.3g, %ld singular values dropped\n",
                                 lu ? "LU" : "SVD pseudo-inverse", (long)n0, resid, (long)dropped);
            } else {
                invert_spd_device(D, n0, stream);
                coarse_inverse.push_back({0, 0.0, 0});
            }
            ao[s] = (int64_t)packed.size();
            no[s] = lev[clev].noff[s];
            nz[s] = n0;
            ldv[s] = coarse_pack(D, subs[s], clev, p, pad64(lev[clev].nloc[s]), packed);
        }
        if (vc32()) {
            // reduced-precision preconditioner storage: the (exactly symmetric) dense inverses in
            // fp32 -- half the bytes of the coarse GEMV, which dominates small batches' coarse time
            std::vector<float> p32(packed.begin(), packed.end());
            ainv32.upload(p32);
        } else
            ainv.upload(packed);
        aoff.upload(ao);
        c_noff.upload(no);
        c_n.upload(nz);
        c_ld.upload(ldv);
        if (tune.verbose)
            std::fprintf(stderr, "[ddpca] exact coarse solve on level %d (%zu doubles of dense inverses)\n", clev, packed.size());
    }

    // ---- work buffers
    // condensed <-> nodal map of the fine level
    const LevelDev& F = lev.back();
    nfree.resize(nsub);
    free_dof_host.resize(nsub);
    free_dof.resize(nsub);
    std::vector<int64_t> cb(nsub + 1, 0);
    for (int s = 0; s < nsub; ++s) {
        free_dof_host[s] = free_dof_map(subs[s], fine_perm[s], F.noff[s]);
        nfree[s] = (int64_t)free_dof_host[s].size();
        free_dof[s].upload(free_dof_host[s]);
        cb[s] = F.noff[s] / kChunk;
    }
    cb[nsub] = F.nch;
    fin_cb.upload(cb);
    {
        // the six PCG vectors in one allocation; DDPCA_STAGGER (doubles) shifts each vector's
        // start so equal indices of z, p, q do not share address bits
#ifdef DDPCA_STAGGER
        const int64_t stag = DDPCA_STAGGER;
#else
        const int64_t stag = 0;
#endif
        const int64_t seg = (3 * F.nn + 511) / 512 * 512 + stag;
        pcg_mem.alloc(6 * seg);
        pcg_mem.zero(stream);
        int i = 0;
        for (auto* v : {&xs, &rs, &zs, &ps, &qs, &bs}) {
            v->p = pcg_mem.p + (i++) * seg;
            v->n = 3 * F.nn;
        }
    }
    int64_t maxch = 0;
    for (auto& L : lev) maxch = std::max<int64_t>(maxch, L.nch);
    partial.alloc(2 * maxch);
    if (gs_fine()) gs.partial.alloc(gs.nchunk);
    if (gs_fine() && opt.precond_fp32 == 4 && !gs.band && lev.back().lat && lev.back().nrot == 0) {
        gs.x4.alloc(4 * lev.back().nn);
        gs.x4.zero(stream);
        if (tune.gs_r32) {  // the residual the restriction reads, in fp32 too
            gs.r4.alloc(4 * lev.back().nn);
            gs.r4.zero(stream);
        }
    }
    // fp32 iterate copies of the block-Jacobi levels (precond_fp32 = 4, block-Jacobi smoothing):
    // every level the V-cycle smooths by block Jacobi whose
    // copy has 16-bit columns and streamed values (rotation block entries into it included) -- its
    // sweeps and residual gather one 16-B load per neighbour, only the level's last sweep writes
    // fp64.  Alternating in one call (profiles/r06n): the N = 8 rank 9.52 / 9.55 -> 9.00 / 9.00 ms
    // per ADMM iteration, the headline 19.73 / 19.74 -> 20.05 / 20.06 ADMM it/s, PCG iterations equal
    if (tune.bj_x4 && opt.precond_fp32 == 4 && (opt.smoother == 1 || opt.smoother >= 3))
        for (int l = clev + 1; l < (int)lev.size(); ++l) {
            LevelDev& L = lev[l];
            if ((gs_fine() && l == (int)lev.size() - 1) || !L.col16.p || L.tbl) continue;
            L.x4a.alloc(4 * L.nn);
            L.x4b.alloc(4 * L.nn);
            L.x4a.zero(stream);
            L.x4b.zero(stream);
        }
    if (gs_fine() && opt.smoother == 4) {
        gs.w.alloc(3 * lev.back().nn);
        gs.w.zero(stream);
    }
    // the colour plan's byte model is smoother 3's on fp64 iterates
    if (gs_fine() && (gs.x4.p || opt.smoother == 4)) colour_byte_model(gs, opt.smoother, gs.x4.p != nullptr, gs.r4.p != nullptr);
    sc.alloc(nsub);
    DDPCA_HIP(hipHostMalloc(reinterpret_cast<void**>(&sc_host), nsub * sizeof(PcgScal)));
    std::memset(sc_host, 0, nsub * sizeof(PcgScal));
    mirror.alloc(nsub);
    DDPCA_HIP(hipEventCreate(&ev_k0));
    DDPCA_HIP(hipEventCreate(&ev_k1));

    // ---- smoother coefficients from the spectrum of M K on each smoothed level and subdomain
    for (int l = 1; l < nlev; ++l) {
        estimate_lmax(l);
        lev[l].coef.upload(smoother_coefs(lev[l].lmax, opt.nu, opt.smoother, opt.omega));
    }
    DDPCA_HIP(hipStreamSynchronize(stream));
}

MgpisDevice::~MgpisDevice() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    for (hipStream_t xs : xstream_)
        if (xs) (void)hipStreamSynchronize(xs);
    for (auto* ga : {graph_, graph1_})
        for (int p = 0; p < 2; ++p)
            if (ga[p]) (void)hipGraphExecDestroy(ga[p]);
    for (auto* gh : {graph_h_, graph1_h_})
        for (int p = 0; p < 2; ++p)
            for (int h = 0; h < kMaxParts; ++h)
                if (gh[p][h]) (void)hipGraphExecDestroy(gh[p][h]);
    if (ev_fork_) (void)hipEventDestroy(ev_fork_);
    for (hipEvent_t e : ev_join_)
        if (e) (void)hipEventDestroy(e);
    for (hipStream_t xs : xstream_)
        if (xs) (void)hipStreamDestroy(xs);
    if (sc_host) (void)hipHostFree(sc_host);
    if (ev_k0) (void)hipEventDestroy(ev_k0);
    if (ev_k1) (void)hipEventDestroy(ev_k1);
    if (stream) (void)hipStreamDestroy(stream);
}

namespace {
// ---- launch dispatch: the one place where a runtime choice of storage becomes a C++ type.  Each
// helper calls the generic callable f with a tag that carries the type; the static exclusions
// (which combinations have a kernel) stay with the caller as if constexpr.
template <typename T>
struct Tag {
    using type = T;
};
template <typename TagT>
using tag_t = typename TagT::type;

// storage type of streamed operator values (ValType)
template <typename F>
void with_val_type(int vt, F&& f) {
    if (vt == kValQ8) f(Tag<uint8_t>{});
    else if (vt == kValH16) f(Tag<uint16_t>{});
    else if (vt == kVal32) f(Tag<float>{});
    else f(Tag<double>{});
}

// column type: 16-bit offsets from the row node where the level or colour copy has them (col16)
template <typename F>
void with_col_type(bool col16, F&& f) {
    if (col16) f(Tag<int16_t>{});
    else f(Tag<int32_t>{});
}

// type of the smoother's inverse: fp32 on levels whose V-cycle copy is reduced precision
template <typename F>
void with_inv_type(bool fp32, F&& f) {
    if (fp32) f(Tag<float>{});
    else f(Tag<double>{});
}
template <typename MT>
const MT* level_minv(const LevelDev& L) {
    if constexpr (std::is_same_v<MT, float>) return L.minv32.p;
    else return L.minv.p;
}

// the smoother's first sweep x = omega M b as the <BJ, SETD, MT> arguments of k_jac0 and of the
// restriction's fused sweep: Chebyshev (block inverse, sets d), block Jacobi, point Jacobi
template <typename F>
void with_first_sweep(bool cheb, bool bj, bool inv32, F&& f) {
    with_inv_type(inv32, [&](auto tm) {
        if (cheb) f(std::true_type{}, std::true_type{}, tm);
        else if (bj) f(std::true_type{}, std::false_type{}, tm);
        else f(std::false_type{}, std::false_type{}, tm);
    });
}
}  // namespace

// lambda_max(M K) per subdomain by 24 power iterations (all subdomains of the batch at once).
void MgpisDevice::estimate_lmax(int l) {
    LevelDev& L = lev[l];
    const bool bj = opt.smoother >= 1;
    const int64_t n = 3 * L.nn;
    std::vector<double> h(n, 0.0);
    std::vector<uint8_t> mask = L.mask.download();
    for (int s = 0; s < nsub; ++s) {
        std::mt19937_64 rng(20251017 + l);
        std::uniform_real_distribution<double> U(-1.0, 1.0);
        for (int64_t i = 3 * L.noff[s]; i < 3 * (L.noff[s] + L.nloc[s]); ++i) h[i] = (mask[i / 3] >> (i % 3)) & 1 ? U(rng) : 0.0;
    }
    DevBuf<double> v, w, scale(nsub);
    v.upload(h);
    w.alloc(n);
    const int nb = ceil_div(L.nn, kBlock);
    std::vector<double> part(L.nch), nrm(nsub), inv(nsub);
    auto norms = [&]() {
        DDPCA_HIP(hipMemcpyAsync(part.data(), partial.p, L.nch * sizeof(double), hipMemcpyDeviceToHost, stream));
        DDPCA_HIP(hipStreamSynchronize(stream));
        for (int s = 0; s < nsub; ++s) {
            double t = 0.0;
            for (int64_t c = L.noff[s] / kChunk; c < (L.noff[s] + pad64(L.nloc[s])) / kChunk; ++c) t += part[c];
            nrm[s] = std::sqrt(t);
            inv[s] = nrm[s] > 0.0 ? 1.0 / nrm[s] : 0.0;
        }
    };
    auto apply_m = [&](const double* x) {
        with_inv_type(vc_type(l) != kVal64, [&](auto tm) {  // the smoother's own inverse (fp32 on reduced levels)
            using MT = tag_t<decltype(tm)>;
            const MT* m = level_minv<MT>(L);
            if (bj) hipLaunchKernelGGL((k_apply_m<true, MT>), dim3(nb), dim3(kBlock), 0, stream, x, m, w.p, partial.p, L.nn);
            else hipLaunchKernelGGL((k_apply_m<false, MT>), dim3(nb), dim3(kBlock), 0, stream, x, m, w.p, partial.p, L.nn);
        });
    };
    apply_m(v.p);
    norms();
    for (int it = 0; it < 24; ++it) {
        // v <- w / |w| ; w <- M K v
        DDPCA_HIP(hipMemcpyAsync(scale.p, inv.data(), nsub * sizeof(double), hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(k_scale_sub, dim3(nb), dim3(kBlock), 0, stream, w.p, scale.p, v.p, L.nn, L.csub.p);
        spmv(l, v.p, L.r.p, true);  // the smoother's operator
        apply_m(L.r.p);
        norms();
    }
    L.lmax.resize(nsub);
    for (int s = 0; s < nsub; ++s) L.lmax[s] = nrm[s] * 1.05;  // safety margin on the estimate
}

// ============================================================================== operations
namespace {
// Krylov-operator arguments (fp64 values) of a level
SellArgs level_args(const LevelDev& L) {
    SellArgs a{};
    a.slots = L.slots.p;
    a.off = L.off.p;
    a.col = L.col.p;
    a.col16 = L.col16.p;
    a.val = L.val.p;
    a.csub = L.csub.p;
    a.nch = L.nch;
    a.minv = L.minv.p;

    if (L.tbl) {
        a.val = nullptr;
        a.rtype = L.rtype.p;
        a.ctype = L.ctype.p;
        a.tab = L.tab.p;
        a.tstride = L.tstride;
    }
    return a;
}

// one SELL launch over a level: table mode when the arguments carry a table, else values
// streamed in storage type vt (kVal64 / kVal32 / kValH16 / kValQ8)
template <int MODE, bool BJ, bool DOT>
void launch_sell(int vt, const SellArgs& a, hipStream_t s) {
    const dim3 grid(ceil_div(a.nch, 4));
    constexpr int V = default_variant(MODE);
    // the V-cycle's sweep and residual: only they have the fp32 iterate copy and the row-split kernel
    constexpr bool VC = MODE == kResid || MODE == kJac;
    // small levels: the row-split kernel (DDPCA_SPLIT_CHUNKS = the largest level it takes, in chunks)
    // (read per launch: launches are captured into graphs once per handle, and tests switch it)
    const char* esp = std::getenv("DDPCA_SPLIT_CHUNKS");
    const int64_t split_max = esp ? std::atoll(esp) : 2048;
    // a block-Jacobi level's fp32 iterate copy (LevelDev::x4a): the constructor enables it
    // on levels with 16-bit columns and streamed values only
    const bool x4 = VC && a.x4;
    if (x4 && (a.tab || !a.col16)) throw ApiError(DDPCA_ESTATE, "fp32 iterate copy needs 16-bit columns and streamed values");
    if (a.tab) {  // table mode: fp64 table, 32-bit columns
        hipLaunchKernelGGL((k_sell<MODE, BJ, DOT, double, V, true>), grid, dim3(kBlock), 0, s, a, a.tab);
        return;
    }
    auto launch = [&](auto tv, auto tc, auto tx4) {
        using T = tag_t<decltype(tv)>;
        using CT = tag_t<decltype(tc)>;
        constexpr bool X4 = decltype(tx4)::value;
        // (V-cycle modes only: y = Kx keeps the slot order the table mode reproduces bit for bit)
        if constexpr (VC && !DOT) {
            if (a.nch <= split_max) {
                hipLaunchKernelGGL((k_sell_split<MODE, BJ, T, CT, X4>), dim3((unsigned)a.nch), dim3(kBlock), 0, s, a);
                return;
            }
        }
        hipLaunchKernelGGL((k_sell<MODE, BJ, DOT, T, V, false, CT, X4>), grid, dim3(kBlock), 0, s, a, a.tab);
    };
    with_val_type(vt, [&](auto tv) {
        if constexpr (VC) {
            if (x4) {
                launch(tv, Tag<int16_t>{}, std::true_type{});
                return;
            }
        }
        with_col_type(a.col16 != nullptr, [&](auto tc) { launch(tv, tc, std::false_type{}); });
    });
}

// one smoothing sweep of the V-cycle: Chebyshev, block Jacobi or point Jacobi, with or without
// the partials of the dot product
void launch_sweep(bool cheb, bool bj, bool dot, int vt, const SellArgs& a, hipStream_t s) {
    auto run = [&](auto tdot) {
        constexpr bool DOT = decltype(tdot)::value;
        if (cheb) launch_sell<kCheb, true, DOT>(vt, a, s);
        else if (bj) launch_sell<kJac, true, DOT>(vt, a, s);
        else launch_sell<kJac, false, DOT>(vt, a, s);
    };
    if (dot) run(std::true_type{});
    else run(std::false_type{});
}

// the same with the loop variant chosen at run time (bench_spmv): 32-bit columns, streamed values
template <int MODE, bool BJ, bool DOT>
void launch_loop(int loop, int vt, const SellArgs& a, int grid, hipStream_t s) {
    with_val_type(vt, [&](auto tv) {
        using T = tag_t<decltype(tv)>;
        switch (loop) {
            case 0: hipLaunchKernelGGL((k_sell<MODE, BJ, DOT, T, 0>), dim3(grid), dim3(kBlock), 0, s, a, a.tab); break;
            case 1: hipLaunchKernelGGL((k_sell<MODE, BJ, DOT, T, 1>), dim3(grid), dim3(kBlock), 0, s, a, a.tab); break;
            case 2: hipLaunchKernelGGL((k_sell<MODE, BJ, DOT, T, 2>), dim3(grid), dim3(kBlock), 0, s, a, a.tab); break;
            default: hipLaunchKernelGGL((k_sell<MODE, BJ, DOT, T, 3>), dim3(grid), dim3(kBlock), 0, s, a, a.tab); break;
        }
    });
}
}  // namespace

namespace {
// V-cycle-operator arguments of a level: the fp32 copy when the preconditioner stores it
SellArgs vc_level_args(const MgpisDevice& D, int level) {
    SellArgs a = level_args(D.lev[level]);
    const int vt = D.vc_type(level);
    const LevelDev& L = D.lev[level];
    if (vt == kValQ8) a.val = L.val8.p;
    else if (vt == kValH16) a.val = L.val16.p;
    else if (vt == kVal32) a.val = L.val32.p;
    if (vt != kVal64) a.minv = L.minv32.p;
    return a;
}
}  // namespace

namespace {
// k_restrict over level l -> l-1 with the transfer's weight form (stored or uniform)
template <bool INIT, bool BJ, bool SETD, typename MT>
void launch_restrict(const LevelDev& F, int grid, hipStream_t st, const double* rf, const uint8_t* cmask, double* bc,
                     double* xc, double* dc, const MT* minv, const double* coef, int64_t nc, const int32_t* csub,
                     const PcgScal* sc, const float4* rf4 = nullptr, float4* xc4 = nullptr) {
    // rf4: the fine residual in the colour sweeps' fp32 copy (lattice transfers only, GsFine::r4);
    // xc4: the fused first coarse sweep writes the coarse level's fp32 iterate copy (LevelDev::x4a)
    if (rf4) {
        if (!F.lat) throw ApiError(DDPCA_ESTATE, "fp32 residual copy without lattice transfers");
        hipLaunchKernelGGL((k_restrict_lat<INIT, BJ, SETD, MT, float4>), dim3(grid), dim3(kBlock), 0, st, rf4, F.rmsk.p,
                           F.rf0.p, F.rstr.p, cmask, bc, xc, dc, minv, coef, nc, csub, sc, xc4);
        return;
    }
    // stored weights: deriving them from a gathered parent count (as k_prolong<true> does)
    // measured 58 -> 102 us on the fine level (profiles/r01_transfer_weights.txt)
    if (F.lat) {
        hipLaunchKernelGGL((k_restrict_lat<INIT, BJ, SETD, MT>), dim3(grid), dim3(kBlock), 0, st, rf, F.rmsk.p, F.rf0.p,
                           F.rstr.p, cmask, bc, xc, dc, minv, coef, nc, csub, sc, xc4);
        return;
    }
    hipLaunchKernelGGL((k_restrict<INIT, BJ, SETD, MT>), dim3(grid), dim3(kBlock), 0, st, rf, F.rslots.p, F.roff.p,
                       F.rcol.p, F.rwt.p, cmask, bc, xc, dc, minv, coef, nc, csub, sc, xc4);
}
}  // namespace

void MgpisDevice::restrict_level(int l, const double* rf, double* bc) {
    if (l < 1 || l >= (int)lev.size()) throw ApiError(DDPCA_EINVAL, "restrict_level: level");
    const LevelDev& F = lev[l];
    const LevelDev& C = lev[l - 1];
    launch_restrict<false, false, false, double>(F, ceil_div(C.nn, kBlock), stream, rf, C.mask.p, bc, nullptr, nullptr,
                                                 nullptr, nullptr, C.nn, C.csub.p, nullptr);
    rot_restrict(l, rf, bc, nullptr);
}

void MgpisDevice::rot_restrict(int l, const double* rf, double* bc, const PcgScal* scp) {
    const LevelDev& F = lev[l];
    if (!F.nrotc) return;
    hipLaunchKernelGGL(k_restrict_rot, dim3(ceil_div(F.nrotc, kBlock)), dim3(kBlock), 0, stream, rf, F.rotc_row.p,
                       F.rotc_ptr.p, F.rotc_kid.p, F.rotc_blk.p, lev[l - 1].mask.p, bc, F.nrotc, lev[l - 1].csub.p, scp);
}

void MgpisDevice::prolong_level(int l, const double* ec, double* xf, float4* xf4, const PcgScal* scp) {
    const LevelDev& F = lev[l];
    const dim3 grid(ceil_div(F.nn, kBlock)), block(kBlock);
    auto into = [&](auto* x) {  // x: the fp64 iterate, or the fp32 copy that takes the correction instead
        using XT = std::remove_pointer_t<decltype(x)>;
        if (F.lat)
            hipLaunchKernelGGL(k_prolong_lat<XT>, grid, block, 0, stream, ec, F.ppk.p, F.pstr.p, F.mask.p, x, F.nn, F.csub.p, scp);
        else if (F.uw)
            hipLaunchKernelGGL((k_prolong<true, XT>), grid, block, 0, stream, ec, F.ppar.p, F.pw.p, F.mask.p, x, F.nn, F.csub.p, scp);
        else
            hipLaunchKernelGGL((k_prolong<false, XT>), grid, block, 0, stream, ec, F.ppar.p, F.pw.p, F.mask.p, x, F.nn, F.csub.p, scp);
        if (F.nrot)  // the block entries' part
            hipLaunchKernelGGL(k_prolong_rot<XT>, dim3(ceil_div(F.nrot, kBlock)), block, 0, stream, ec, F.rot_row.p,
                               F.rot_ptr.p, F.rot_par.p, F.rot_blk.p, F.mask.p, x, F.nrot, F.csub.p, scp);
    };
    if (xf4) into(xf4);
    else into(xf);
}

void MgpisDevice::first_sweep(int l, const double* b, const double* cf, double* x, float4* x4, const PcgScal* scp) {
    const LevelDev& L = lev[l];
    with_first_sweep(opt.smoother == 2, opt.smoother >= 1, vc_type(l) != kVal64, [&](auto bj, auto setd, auto tm) {
        using MT = tag_t<decltype(tm)>;
        constexpr bool BJ = decltype(bj)::value, SETD = decltype(setd)::value;
        hipLaunchKernelGGL((k_jac0<BJ, SETD, MT>), dim3(ceil_div(L.nn, kBlock)), dim3(kBlock), 0, stream, b,
                           level_minv<MT>(L), cf, x, SETD ? L.d.p : nullptr, L.nn, L.csub.p, scp, x4);
    });
}

void MgpisDevice::coarse_solve(const double* b, double* x, const PcgScal* scp) {
    const LevelDev& C = lev[clev];
    const dim3 grid(ceil_div(3 * C.nn, 4));
    if (ainv32.p)
        hipLaunchKernelGGL(k_coarse<float>, grid, dim3(kBlock), 0, stream, ainv32.p, aoff.p, c_noff.p, c_n.p, c_ld.p, b, x,
                           3 * C.nn, C.csub.p, scp);
    else
        hipLaunchKernelGGL(k_coarse<double>, grid, dim3(kBlock), 0, stream, ainv.p, aoff.p, c_noff.p, c_n.p, c_ld.p, b, x,
                           3 * C.nn, C.csub.p, scp);
}

void MgpisDevice::restrict_into(int c, const float4* rf4, double* xc, float4* xc4, const PcgScal* scp) {
    const LevelDev& F = lev[c + 1];
    const LevelDev& C = lev[c];
    const int grid = ceil_div(C.nn, kBlock);
    const double* cf = c > 0 ? lev[c].coef.p : nullptr;  // the first sweep's (c1, c2)
    auto plain = [&](const float4* r4) {
        launch_restrict<false, false, false, double>(F, grid, stream, F.r.p, C.mask.p, C.b.p, nullptr, nullptr, nullptr,
                                                     nullptr, C.nn, C.csub.p, scp, r4);
    };
    if (F.nrot) {
        // block transfer entries: plain restriction, the blocks' B^T part, then the first
        // coarse sweep x_c = omega M b_c that k_restrict otherwise fuses
        plain(nullptr);
        rot_restrict(c + 1, F.r.p, C.b.p, scp);
        if (c != clev) first_sweep(c, C.b.p, cf, xc, xc4, scp);
    } else if (c == clev) {
        plain(rf4);
    } else {
        with_first_sweep(opt.smoother == 2, opt.smoother >= 1, vc_type(c) != kVal64, [&](auto bj, auto setd, auto tm) {
            using MT = tag_t<decltype(tm)>;
            constexpr bool BJ = decltype(bj)::value, SETD = decltype(setd)::value;
            launch_restrict<true, BJ, SETD, MT>(F, grid, stream, F.r.p, C.mask.p, C.b.p, xc, SETD ? C.d.p : nullptr,
                                                level_minv<MT>(C), cf, C.nn, C.csub.p, scp, rf4, xc4);
        });
    }
}

void MgpisDevice::spmv(int level, const double* x, double* y, bool vc_op) {
    SellArgs a = vc_op ? vc_level_args(*this, level) : level_args(lev[level]);
    if (!a.val && !a.tab) throw ApiError(DDPCA_ESTATE, "operator of this level is not stored in the requested precision");
    a.x = x;
    a.y = y;
    launch_sell<kSpmv, false, false>(vc_op ? vc_type(level) : kVal64, a, stream);
}

double MgpisDevice::bench_spmv(int variant, int reps) {
    // variant = loop (0..3) + 4 * mode (0 y = Kx, 1 PCG, 2 residual, 3 Chebyshev sweep) + 16 *
    // fp32 values (the V-cycle copy); fine level, whole batch, operands in the PCG work vectors
    // (values are irrelevant to the timing)
    // table-mode levels (y = Kx only): + 32 selects the table diagnostics, loop 0 per-lane
    // table rows, 1 production, 3 coalesced-x bound, 32 + 0/1 x stride 4 (16+8 B / 2x16 B loads)
    const LevelDev& L = lev.back();
    const int loop = variant & 3, mode = (variant >> 2) & 3;
    const bool f32 = (variant & 16) != 0;
    const int vt = !f32 ? kVal64 : vc_type((int)lev.size() - 1);  // the V-cycle's copy
    const int tloop = (variant & 32) ? 4 + (loop & 1) : loop;
    if (variant >= 64 || ((variant & 32) && (!L.tbl || mode != 0 || f32))) throw ApiError(DDPCA_EINVAL, "unknown SpMV variant");
    if (mode == 3 && (lev.size() < 2 || opt.smoother < 1)) throw ApiError(DDPCA_EINVAL, "Chebyshev mode needs block smoothing");
    if (f32 && !L.val32.p && !L.val16.p && !L.val8.p) throw ApiError(DDPCA_EINVAL, "no reduced-precision operator (precond_fp32 = 0)");
    DDPCA_HIP(hipMemsetAsync(sc.p, 0, nsub * sizeof(PcgScal), stream));  // done = 0, beta = 0
    SellArgs a = level_args(L);
    if (f32) {
        a.val = vc_level_args(*this, (int)lev.size() - 1).val;
        a.tab = nullptr;
    }
    a.x = xs.p;
    a.y = qs.p;
    a.p = ps.p;
    a.b = bs.p;
    a.xo = rs.p;
    a.partial = partial.p;
    a.sc = sc.p;
    if (lev.size() > 1) a.coef = L.coef.p;
    const int grid = ceil_div(a.nch, 4);
    DevBuf<double> x4;
    if (tloop >= 4) {  // x in a 4-double-per-node copy
        x4.alloc(4 * L.nn);
        DDPCA_HIP(hipMemcpy2DAsync(x4.p, 32, xs.p, 24, 24, L.nn, hipMemcpyDeviceToDevice, stream));
        a.x = x4.p;
    }
    auto table_variant = [&](auto v) {  // y = Kx from the table, diagnostic loop variant v
        hipLaunchKernelGGL((k_sell<kSpmv, false, false, double, decltype(v)::value, true>), dim3(grid), dim3(kBlock), 0,
                           stream, a, a.tab);
    };
    auto in_mode = [&](auto m, auto bj, auto dot) {
        constexpr int MODE = decltype(m)::value;
        constexpr bool BJ = decltype(bj)::value, DOT = decltype(dot)::value;
        if (a.tab) launch_sell<MODE, BJ, DOT>(kVal64, a, stream);  // table mode: one loop variant
        else launch_loop<MODE, BJ, DOT>(loop, vt, a, grid, stream);
    };
    using std::integral_constant;
    auto launch = [&]() {
        if (a.tab && mode == 0 && tloop != 1) {
            switch (tloop) {
                case 0: table_variant(integral_constant<int, 0>{}); break;
                case 3: table_variant(integral_constant<int, 3>{}); break;
                case 4: table_variant(integral_constant<int, 4>{}); break;
                case 5: table_variant(integral_constant<int, 5>{}); break;
                default: table_variant(integral_constant<int, 2>{}); break;
            }
        } else if (mode == 0) in_mode(integral_constant<int, kSpmv>{}, std::false_type{}, std::false_type{});
        else if (mode == 1) in_mode(integral_constant<int, kPcg>{}, std::false_type{}, std::true_type{});
        else if (mode == 2) in_mode(integral_constant<int, kResid>{}, std::false_type{}, std::false_type{});
        else in_mode(integral_constant<int, kCheb>{}, std::true_type{}, std::false_type{});
    };
    launch();
    DDPCA_HIP(hipEventRecord(ev_k0, stream));
    for (int r = 0; r < reps; ++r) launch();
    DDPCA_HIP(hipEventRecord(ev_k1, stream));
    DDPCA_HIP(hipEventSynchronize(ev_k1));
    float ms = 0.f;
    DDPCA_HIP(hipEventElapsedTime(&ms, ev_k0, ev_k1));
    return (double)ms / std::max(reps, 1);
}

namespace {
// the colour copy the sweeps stream: its storage type and values (GsFine holds exactly one)
std::pair<int, const void*> gs_values(const GsFine& G) {
    if (G.val8.p) return {kValQ8, G.val8.p};
    if (G.val16.p) return {kValH16, G.val16.p};
    if (G.val32.p) return {kVal32, G.val32.p};
    return {kVal64, G.val64.p};
}

// one colour-sweep launch: phase PH (k_gs, 6..10 k_gs_ssor) over the chunks k selects.
// k >= 0: colour k; k = -1: every colour chunk (the residual); band mode: k = -2 the ring group,
// k = -3 the ring and far groups (PH 3..5 run k_gs_aux)
template <int PH, bool DOT>
void launch_gs(const MgpisDevice& D, int k, double* x, const double* b, double* r, const PcgScal* scp, double* partial) {
    const GsFine& G = D.gs;
    const LevelDev& F = D.lev.back();
    const int K = G.ncol;
    GsArgs a{};
    if (k >= 0) {
        a.list = G.list.p + G.first[k];
        a.n = G.count[k];
    } else if (k == -1) {
        a.list = G.band ? G.list.p : nullptr;
        a.n = G.band ? G.first[K] : G.nchunk;
    } else {
        if (!G.band) throw ApiError(DDPCA_ESTATE, "ring / far chunk groups without band mode");
        a.list = G.list.p + G.first[K];
        a.n = G.count[K] + (k == -3 ? G.count[K + 1] : 0);
    }
    if (a.n == 0) return;
    a.rowidx = G.rowidx.p;
    a.csub = G.csub.p;
    a.nsl = G.nsl.p;
    a.nsu = G.nsu.p;
    a.offl = G.offl.p;
    a.offu = G.offu.p;
    a.col = G.col.p;
    a.col16 = G.col16.p;
    a.x = x;
    a.b = b;
    a.r = r;
    a.sc = scp;
    a.partial = partial;
    // the rows' fp32 inverses in chunk order (coalesced: read by row at stride 2 nodes they pulled
    // whole lines for half the data, +1.1 %, profiles/r03o); the fp64 copy reads minv by row
    a.minvc = G.minvc.p;
    a.x4 = reinterpret_cast<float4*>(G.x4.p);
    a.r4 = reinterpret_cast<float4*>(G.r4.p);
    a.w = G.w.p;
    const auto [vt, val] = gs_values(G);
    a.val = val;
    if (vt != kVal64) a.minv = F.minv32.p;
    else a.minv = F.minv.p;
    // SSOR phases: the reduced-precision copies' chunk-ordered inverses
    if (PH >= 6 && (!G.minvc.p || vt == kVal64))
        throw ApiError(DDPCA_ESTATE, "colour SSOR needs a reduced-precision V-cycle copy (precond_fp32 >= 1)");
    const dim3 grid((unsigned)a.n);
    with_val_type(vt, [&](auto tv) {
        with_col_type(G.col16.p != nullptr, [&](auto tc) {
            using T = tag_t<decltype(tv)>;
            using CT = tag_t<decltype(tc)>;
            if constexpr (PH >= 6) {
                if constexpr (!std::is_same_v<T, double>) {
                    if (a.x4) hipLaunchKernelGGL((k_gs_ssor<PH, DOT, T, CT, true>), grid, dim3(kWave), 0, D.stream, a);
                    else hipLaunchKernelGGL((k_gs_ssor<PH, DOT, T, CT>), grid, dim3(kWave), 0, D.stream, a);
                    return;
                }
            }
            // (no else: as before, the code object also carries k_gs_aux<6..10>, which nothing launches)
            if constexpr (PH >= 3) {  // the band mode's ring / far groups
                hipLaunchKernelGGL((k_gs_aux<PH, T, CT>), grid, dim3(kWave), 0, D.stream, a);
            } else {
                if (a.x4) hipLaunchKernelGGL((k_gs<PH, DOT, T, CT, true>), grid, dim3(kWave), 0, D.stream, a);
                else hipLaunchKernelGGL((k_gs<PH, DOT, T, CT>), grid, dim3(kWave), 0, D.stream, a);
            }
        });
    });
}
}  // namespace

void MgpisDevice::vcycle(const double* rin, double* zout, bool dot) {
    if (no_coarse) throw ApiError(DDPCA_ESTATE, "one-level handle without a coarse inverse: diagonal preconditioner only");
    const int nlev = (int)lev.size();
    const int Lf = nlev - 1;
    const bool bj = opt.smoother >= 1;
    const bool cheb = opt.smoother == 2;
    const int nu = opt.nu;
    const PcgScal* scp = sc_cur_ ? sc_cur_ : sc.p;
    const int cl = clev;  // the exact dense solve; levels below it are not visited
    if (Lf == cl) {
        coarse_solve(rin, zout, scp);
        if (dot)
            hipLaunchKernelGGL(k_dot, dim3(ceil_div(lev[cl].nn, kBlock)), dim3(kBlock), 0, stream, rin, zout, partial.p,
                               lev[cl].nn, lev[cl].csub.p, scp);
        return;
    }
    std::vector<double*> cur(nlev), oth(nlev);
    for (int l = 0; l < nlev; ++l) { cur[l] = lev[l].x.p; oth[l] = lev[l].t.p; }
    cur[Lf] = lev[Lf].t.p;
    oth[Lf] = zout;
    // block-Jacobi levels with fp32 iterate copies (LevelDev::x4a / x4b, precond_fp32 = 4): their
    // first sweep, the sweeps and the prolongation into them write the copy, the sweeps and the
    // residual gather it, and only the level's last sweep writes its fp64 iterate
    std::vector<float4*> cur4(nlev, nullptr), oth4(nlev, nullptr);
    for (int l = 0; l < nlev; ++l)
        if (lev[l].x4a.p) {
            cur4[l] = reinterpret_cast<float4*>(lev[l].x4a.p);
            oth4[l] = reinterpret_cast<float4*>(lev[l].x4b.p);
        }
    auto bvec = [&](int l) -> const double* { return l == Lf ? rin : lev[l].b.p; };
    auto coef = [&](int l, int sweep) { return lev[l].coef.p + 2 * (int64_t)sweep * nsub; };
    // smoothing sweeps on level l from the current iterate (first: jac0/restrict already did sweep 0);
    // out64: the last of them is the level's output (fp64 also on an fp32-copy level)
    auto smooth = [&](int l, int first, int count, bool last_dot, bool out64) {
        const int vt = vc_type(l);
        for (int s = first; s < first + count; ++s) {
            SellArgs a = vc_level_args(*this, l);
            a.sc = scp;
            a.partial = partial.p;
            a.x = cur[l];
            a.b = bvec(l);
            a.xo = oth[l];
            a.coef = coef(l, s);
            if (cur4[l]) {
                const bool fin = out64 && s == first + count - 1;
                a.x4 = cur4[l];
                a.xo4 = fin ? nullptr : oth4[l];
                a.xo = fin ? oth[l] : nullptr;
            }
            const bool d = last_dot && s == first + count - 1;
            if (cheb) a.p = lev[l].d.p;
            launch_sweep(cheb, bj, d, vt, a, stream);
            std::swap(cur[l], oth[l]);
            std::swap(cur4[l], oth4[l]);
        }
    };
    const bool gsf = gs_fine();
    if (gsf) cur[Lf] = zout;  // the Gauss-Seidel sweeps run in place
    // ---- descend
    const bool ssor = gsf && opt.smoother == 4;
    if (ssor) {
        // colour SSOR: forward sweep from zero, backward sweep, residual r = w - L x
        for (int k = 0; k < gs.ncol; ++k) launch_gs<6, false>(*this, k, zout, rin, nullptr, scp, nullptr);
        for (int k = gs.ncol - 1; k >= 0; --k) launch_gs<7, false>(*this, k, zout, rin, nullptr, scp, nullptr);
        launch_gs<8, false>(*this, -1, zout, rin, lev[Lf].r.p, scp, nullptr);
    } else if (gsf) {
        // forward sweep from zero, colour by colour, then r = -U x in one launch; band mode: the
        // rows outside the colours start at x = 0, r = b, the ring's r = b - K x after the sweep
        if (gs.band) launch_gs<5, false>(*this, -3, zout, rin, lev[Lf].r.p, scp, nullptr);
        for (int k = 0; k < gs.ncol; ++k) launch_gs<0, false>(*this, k, zout, rin, nullptr, scp, nullptr);
        launch_gs<1, false>(*this, -1, zout, nullptr, lev[Lf].r.p, scp, nullptr);
        if (gs.band) launch_gs<3, false>(*this, -2, zout, rin, lev[Lf].r.p, scp, nullptr);
    } else {
        first_sweep(Lf, rin, coef(Lf, 0), cur[Lf], cur4[Lf], scp);
    }
    for (int l = Lf; l >= cl + 1; --l) {
        if (!(gsf && l == Lf)) {
            smooth(l, 1, nu - 1, false, false);
            SellArgs a = vc_level_args(*this, l);
            a.sc = scp;
            a.x = cur[l];
            a.x4 = cur4[l];
            a.b = bvec(l);
            a.y = lev[l].r.p;
            launch_sell<kResid, false, false>(vc_type(l), a, stream);
        }
        // x4 mode: the colour sweeps' residual is the fp32 copy (GsFine::r4)
        const float4* rf4 = gsf && l == Lf && gs.r4.p ? reinterpret_cast<const float4*>(gs.r4.p) : nullptr;
        restrict_into(l - 1, rf4, cur[l - 1], cur4[l - 1], scp);
    }
    coarse_solve(lev[cl].b.p, cur[cl], scp);
    // ---- ascend
    for (int l = cl + 1; l <= Lf; ++l) {
        // x4 mode (GsFine::x4: lattice fine transfer, no block entries): into the colour sweeps'
        // fp32 copy; a block-Jacobi level's fp32 copy likewise takes the correction
        float4* x4 = gsf && l == Lf && gs.x4.p ? reinterpret_cast<float4*>(gs.x4.p) : cur4[l];
        prolong_level(l, cur[l - 1], cur[l], x4, scp);
        if (ssor && l == Lf) {
            // colour SSOR after the coarse correction: forward, then backward with the dot partials
            for (int k = 0; k < gs.ncol; ++k) launch_gs<9, false>(*this, k, zout, rin, nullptr, scp, nullptr);
            for (int k = gs.ncol - 1; k >= 0; --k) {
                if (dot) launch_gs<10, true>(*this, k, zout, rin, nullptr, scp, gs.partial.p);
                else launch_gs<10, false>(*this, k, zout, rin, nullptr, scp, nullptr);
            }
            continue;
        }
        if (gsf && l == Lf) {
            // backward sweep; the dot product's partials per colour chunk (vc_cb)
            for (int k = gs.ncol - 1; k >= 0; --k) {
                if (dot) launch_gs<2, true>(*this, k, zout, rin, nullptr, scp, gs.partial.p);
                else launch_gs<2, false>(*this, k, zout, rin, nullptr, scp, nullptr);
            }
            // band mode: the dot product's partials of the rows outside the colours
            if (dot && gs.band) launch_gs<4, false>(*this, -3, zout, rin, nullptr, scp, gs.partial.p);
            continue;
        }
        // post-smoothing restarts the smoother (Chebyshev recurrence) from the prolongated iterate
        smooth(l, 0, nu, dot && l == Lf, true);
    }
    if (cur[Lf] != zout) throw ApiError(DDPCA_ESTATE, "V-cycle buffer parity");
}

double MgpisDevice::fine_matrix_bytes(int s, int vt, bool prod_cols) const {
    // operator bytes one fine-level pass reads for member s: streamed values = 4 B index + 72 B
    // (fp64), 36 B (fp32), 20 B (block-exponent fp16) or 10 B (block-scaled int8) per stored block; table mode = 4 B index per block +
    // 4 B row type per node + the member's share of the table (read once per launch)
    const LevelDev& L = lev.back();
    // (the production kernels read 2-B column offsets where the level has them, prod_cols)
    const double cb = (prod_cols && L.col16.p) ? 2.0 : 4.0;
    if (!L.tbl) return (cb + vbytes(vt)) * (double)L.nnzb_sub[s];
    double nodes = 0.0;
    for (int64_t n : L.nloc) nodes += (double)n;
    return 4.0 * (double)L.nnzb_sub[s] + 4.0 * (double)L.nloc[s] +
           (double)L.ntypes * (double)L.tstride * 8.0 * (double)L.nloc[s] / nodes;
}

double MgpisDevice::fine_kernel_bytes(int s) const {
    // algorithmic bytes of one fine-level k_sell<kPcg> for member s: the operator + z gathered
    // once (24 B/node) + p, q read and written (4 x 24 B/node)
    return fine_matrix_bytes(s, kVal64) + 24.0 * 5.0 * (double)lev.back().nloc[s];
}

// ---- algorithmic byte model of the solve path (per member s; bytes every kernel must move at
// least once: streamed operator values + column indices, each vector read / written once, a
// gathered vector counted once per element).  The launch sequence is the one vcycle() and
// enqueue_iteration() issue; the sizes are the member's real (unpadded) nodes.

void MgpisDevice::vcycle_bytes(int s, double out[2]) const {
    out[0] = out[1] = 0.0;
    const int nlev = (int)lev.size(), Lf = nlev - 1, cl = clev;
    const bool bj = opt.smoother >= 1, cheb = opt.smoother == 2;
    auto n = [&](int l) { return (double)lev[l].nloc[s]; };
    auto mat = [&](int l) {  // one pass over the V-cycle's copy of level l
        const LevelDev& L = lev[l];
        if (L.tbl) return 4.0 * (double)L.nnzb_sub[s] + 4.0 * n(l);
        const double cb = L.col16.p ? 2.0 : 4.0;
        return (vbytes(vc_type(l)) + cb) * (double)L.nnzb_sub[s];
    };
    auto minv = [&](int l) { return (bj ? 9.0 : 3.0) * (vc_type(l) != kVal64 ? 4.0 : 8.0); };
    auto put = [&](int l, double b) { out[l == Lf ? 0 : 1] += b; };
    // x' = x + w M (b - K x): operator, x gathered, b, M^-1, x' (Chebyshev: d read + written); on a
    // level with fp32 iterate copies x is gathered in 16 B and x' written in 16 B, in fp64 by the
    // level's last sweep (fin)
    auto x4 = [&](int l) { return lev[l].x4a.p != nullptr; };
    auto sweep = [&](int l, bool fin = true) {
        if (x4(l)) return mat(l) + n(l) * (16.0 + 24.0 + (fin ? 24.0 : 16.0) + minv(l));
        return mat(l) + n(l) * (24.0 * 3 + minv(l) + (cheb ? 48.0 : 0.0));
    };
    const double n0 = 3.0 * (double)lev[cl].nloc[s];
    const double coarse = (ainv32.p ? 4.0 : 8.0) * n0 * n0 + 16.0 * n0;  // dense inverse + b in, x out
    if (Lf == cl) {
        out[0] += coarse + 16.0 * n0;  // + the dot product's second read
        return;
    }
    const bool gsf = gs_fine();
    // multicolour sweeps on the fine level: L + U = the off-diagonal blocks, read once by the
    // forward sweep + residual pair and once by the backward sweep; per launch the x entries of
    // the colours it reads (forward colour k: the k earlier ones, residual: the later ones,
    // backward: all others), and per row b, M^-1, the row index and x (or r) written
    const double K = gsf ? (double)gs.ncol : 0.0;
    const double gsvb = gsf ? vbytes(vc_type(Lf)) + (gs.col16.p ? 2.0 : 4.0) : 0.0;
    const double gsmat = gsvb * (gsf ? (double)gs.nnzb_sub[s] : 0.0);
    // rows the colours sweep (all of them unless band mode), and band mode's ring and far rows
    const double nsw = gsf && gs.band ? (double)gs.band_rows_sub[s] : n(Lf);
    const double nring = gsf && gs.band ? (double)gs.ring_rows_sub[s] : 0.0;
    const double nout = gsf && gs.band ? nring + (double)gs.far_rows_sub[s] : 0.0;
    // x4 mode (GsFine::x4): the iterate the sweeps gather and the forward sweep / prolongation
    // write is the 16-B fp32 copy; the backward sweep writes it and the fp64 output
    const double xb = gsf && gs.x4.p ? 16.0 : 24.0;
    const double rb = gsf && gs.r4.p ? 16.0 : 24.0;  // the residual written by the sweeps, read by the restriction
    const bool ssor = gsf && opt.smoother == 4;
    if (ssor) {
        // colour SSOR: forward from zero (L; b, M^-1, x, w written), backward (U; b, w, M^-1 read, x
        // written), residual (L; w read, r written); x entries gathered as the Gauss-Seidel pair's
        const double lpass = gsmat * 0.5, upass = gsmat * 0.5, row = 4.0;
        put(Lf, lpass + nsw * (24.0 + minv(Lf) + xb + 24.0 + row + xb * (K - 1.0) / 2.0));
        put(Lf, upass + nsw * (48.0 + minv(Lf) + xb + row + xb * (K - 1.0) / 2.0));
        put(Lf, lpass + nsw * (24.0 + rb + row + xb * (K - 1.0) / 2.0));
    } else if (gsf) {
        put(Lf, 76.0 * nout);  // band mode: x = 0, r = b outside the colours (b read, x, r written, row index)
        put(Lf, gsmat + nsw * (24.0 + minv(Lf) + xb + 4.0 + xb * (K - 1.0) / 2.0));  // forward
        put(Lf, nsw * (rb + 4.0 + xb * (K - 1.0) / 2.0));                            // residual
        // band mode: the ring's residual over its band columns (blocks, b read, r written, x gathered)
        put(Lf, gsvb * (double)(gs.band ? gs.ring_nnzb_sub[s] : 0) + nring * (24.0 + 24.0 + 4.0 + 24.0));
    } else {
        put(Lf, n(Lf) * ((x4(Lf) ? 40.0 : 48.0) + minv(Lf) + (cheb ? 24.0 : 0.0)));  // k_jac0: b in, x out
    }
    for (int l = Lf; l >= cl + 1; --l) {
        if (!(gsf && l == Lf)) {
            for (int k = 1; k < opt.nu; ++k) put(l, sweep(l, false));
            put(l, mat(l) + (x4(l) ? 64.0 : 72.0) * n(l));  // residual: x gathered, b, r
        }
        const LevelDev& F = lev[l];
        const int c = l - 1;
        const bool init = c != cl;
        // coarse node: mask + b_c written (+ x_c = w M b_c: M^-1 read, x_c written; Chebyshev d_c)
        double cn = 1.0 + 24.0 + (init ? minv(c) + (x4(c) ? 16.0 : 24.0) + (cheb ? 24.0 : 0.0) : 0.0);
        double tr = (gsf && l == Lf ? rb : 24.0) * n(l);  // r_f read once
        if (F.lat) cn += 8.0;     // 27-bit child mask + fine copy
        else tr += 12.0 * (double)F.tent_sub[s];  // child index + weight per stencil entry
        tr += 4.0 * 8.0 * (double)F.tblk_sub[s] + (F.tblk_sub[s] ? 24.0 * n(c) : 0.0);  // block entries (B^T r_f)
        put(l, tr + cn * n(c));
    }
    put(cl, coarse);
    for (int l = cl + 1; l <= Lf; ++l) {
        const LevelDev& F = lev[l];
        // x_f += mask P e_c: e_c read once, mask, x_f read + written, the parent encoding
        double pb = 24.0 * n(l - 1) + n(l) * (1.0 + (gsf && l == Lf ? 2.0 * xb : x4(l) ? 32.0 : 48.0));
        if (F.lat) pb += 4.0 * n(l);
        else pb += (F.uw ? 4.0 : 12.0) * (double)F.tent_sub[s];
        pb += 4.0 * 8.0 * (double)F.tblk_sub[s];
        put(l, pb);
        if (ssor && l == Lf) {
            // forward from the prolongated x (L + U; b, M^-1 read, x, w written), backward (U; b, w,
            // M^-1 read, z written)
            put(l, gsmat + nsw * (24.0 + minv(l) + xb + 24.0 + 4.0 + xb * (K - 1.0)));
            put(l, gsmat * 0.5 + nsw * (48.0 + minv(l) + 24.0 + 4.0 + xb * (K - 1.0) / 2.0));
            continue;
        }
        if (gsf && l == Lf) {
            put(l, gsmat + nsw * (24.0 + minv(l) + 24.0 + (xb < 24.0 ? xb : 0.0) + 4.0 + xb * (K - 1.0)));  // backward
            put(l, 52.0 * nout);  // band mode: b . x of the rows outside the colours (b, x read, row index)
            continue;
        }
        for (int k = 0; k < opt.nu; ++k) put(l, sweep(l, k == opt.nu - 1));
    }
}

void MgpisDevice::iteration_bytes(int s, double out[2]) const {
    vcycle_bytes(s, out);
    const LevelDev& F = lev.back();
    const double n = (double)F.nloc[s], nch = (double)pad64(F.nloc[s]) / kChunk;
    out[0] += fine_kernel_bytes(s) + 144.0 * n;  // k_sell<kPcg> + k_axpy (x, r read + written, p, q read)
    out[1] += 3.0 * 8.0 * nch;                   // three k_fin passes over the chunk partials
}

void MgpisDevice::setup_bytes(int s, double out[2]) const {
    vcycle_bytes(s, out);
    const LevelDev& F = lev.back();
    const double n = (double)F.nloc[s], nch = (double)pad64(F.nloc[s]) / kChunk;
    out[0] += 120.0 * n;  // k_pcg_init: b read, x r p q written
    out[1] += 2.0 * 8.0 * nch;
}

int64_t MgpisDevice::iteration_launches() const {
    // k_sell<kPcg>, k_axpy, 3 x k_fin, and the V-cycle: jac0 + per descended level (nu - 1 sweeps,
    // residual, restriction) + coarse + per ascended level (prolongation, nu sweeps); the
    // multicolour fine level: one forward and one backward launch per colour + the residual in
    // place of jac0, nu - 1 + 1 + nu sweep launches
    const int64_t nd = (int64_t)lev.size() - 1 - clev;
    const int64_t base = 5 + (nd == 0 ? 2 : 1 + nd * (opt.nu + 1) + 1 + nd * (1 + opt.nu));
    // (band mode: + the x = 0 / r = b launch, the ring's residual and the dot of the other rows)
    if (gs_fine() && nd > 0 && opt.smoother == 4) return base - 1 - 2 * opt.nu + 4 * gs.ncol + 1;  // colour SSOR
    return gs_fine() && nd > 0 ? base - 1 - 2 * opt.nu + 2 * gs.ncol + 1 + (gs.band ? 3 : 0) : base;
}

// k_fin over every member
void MgpisDevice::launch_fin(hipStream_t st, int what, const double* part, const double* part2, const int64_t* cb,
                             PcgScal* scp, PcgMirror* mir) {
    hipLaunchKernelGGL(k_fin, dim3(nsub), dim3(kFinT), 0, st, what, part, part2, cb, scp, mir);
}

void MgpisDevice::enqueue_iteration(int prec, bool timed) {
    LevelDev& L = lev.back();
    PcgScal* scp = sc_cur_ ? sc_cur_ : sc.p;
    SellArgs a = level_args(L);
    a.x = zs.p;
    a.y = qs.p;
    a.p = ps.p;
    a.sc = scp;
    a.partial = partial.p;
    const int nblk = ceil_div(L.nn, kBlock);
    if (timed) DDPCA_HIP(hipEventRecord(ev_k0, stream));
    launch_sell<kPcg, false, true>(kVal64, a, stream);
    if (timed) DDPCA_HIP(hipEventRecord(ev_k1, stream));
    launch_fin(stream, (int)kFinAlpha, partial.p, nullptr, fin_cb.p, scp, mirror.dev);
    hipLaunchKernelGGL(k_axpy, dim3(nblk), dim3(kBlock), 0, stream, xs.p, rs.p, ps.p, qs.p, scp, partial.p, L.nn, L.csub.p);
    launch_fin(stream, (int)kFinRR, partial.p, nullptr, fin_cb.p, scp, mirror.dev);
    if (prec == 1) vcycle(rs.p, zs.p, true);
    else hipLaunchKernelGGL(k_diag, dim3(nblk), dim3(kBlock), 0, stream, rs.p, L.dinv.p, zs.p, partial.p, L.nn, L.csub.p, scp);
    launch_fin(stream, (int)kFinBeta, prec == 1 ? vc_partial() : partial.p, nullptr, prec == 1 ? vc_cb() : fin_cb.p, scp,
               mirror.dev);
}

// graph_[prec]: iters_per_graph PCG iterations captured once and replayed; graph1_[prec]: one.
hipGraphExec_t MgpisDevice::capture_iterations(int prec, int count, PcgScal* scp) {
    sc_cur_ = scp;
    struct Unbind {
        PcgScal*& p;
        ~Unbind() { p = nullptr; }
    } unbind{sc_cur_};  // on a throw out of the capture too
    return capture_graph(stream, [&] {
        for (int k = 0; k < count; ++k) enqueue_iteration(prec, false);
    });
}

void MgpisDevice::build_graph(int prec) {
    if (split_) {
        for (int h = 0; h < nparts_; ++h) build_half_graph(prec, h);
        return;
    }
    if (graph_[prec]) return;
    graph_[prec] = capture_iterations(prec, opt.iters_per_graph, nullptr);
    if (opt.iters_per_graph > 1) graph1_[prec] = capture_iterations(prec, 1, nullptr);
}

// the same iterations bound to half h's copy of the scalars (captured on `stream`, replayed on
// the half's own stream)
void MgpisDevice::build_half_graph(int prec, int h) {
    if (graph_h_[prec][h]) return;
    graph_h_[prec][h] = capture_iterations(prec, opt.iters_per_graph, sc_half_.p + (int64_t)h * nsub);
    if (opt.iters_per_graph > 1) graph1_h_[prec][h] = capture_iterations(prec, 1, sc_half_.p + (int64_t)h * nsub);
}

int64_t MgpisDevice::horizon(int prec, int half) const {
    // DDPCA_TAIL_PACING=0: whole replays to the end (A/B)
    const char* e = std::getenv("DDPCA_TAIL_PACING");
    if ((e && std::atoi(e) == 0) || (int)expect_[prec].size() != nsub) return INT64_MAX;
    int64_t h = 0;
    for (int s = 0; s < nsub; ++s) {
        if (half >= 0 && half_host_[s] != half) continue;
        if (expect_[prec][s] <= 0) return INT64_MAX;
        h = std::max(h, expect_[prec][s]);
    }
    return h;
}

// scs[h][s] = sc[s], with done forced on the members of the other parts
__global__ void k_split_sc(const PcgScal* sc, PcgScal* scs, const int32_t* half, int nsub, int np) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nsub) return;
    for (int h = 0; h < np; ++h) {
        PcgScal v = sc[s];
        if (half[s] != h) v.done = 1;
        scs[h * nsub + s] = v;
    }
}

// sc[s] = the copy of the half that ran member s
__global__ void k_merge_sc(PcgScal* sc, const PcgScal* scs, const int32_t* half, int nsub) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < nsub) sc[s] = scs[half[s] * nsub + s];
}

void MgpisDevice::set_split(bool on, int parts) {
    select_device(device);
    if (on && (parts < 2 || parts > kMaxParts)) throw ApiError(DDPCA_EINVAL, "set_split: 2 .. 4 parts");
    parts = std::min<int>(parts, (int)nsub);
    on = on && nsub >= 2 && !no_coarse;
    if (on == split_ && (!on || parts == nparts_)) return;
    if (split_ && on) throw ApiError(DDPCA_ESTATE, "set_split: the part count is fixed once split");
    DDPCA_HIP(hipStreamSynchronize(stream));
    if (on && !xstream_[0]) {
        nparts_ = parts;
        for (int h = 0; h + 1 < parts; ++h) {
            DDPCA_HIP(hipStreamCreateWithFlags(&xstream_[h], hipStreamNonBlocking));
            DDPCA_HIP(hipEventCreateWithFlags(&ev_join_[h], hipEventDisableTiming));
        }
        DDPCA_HIP(hipEventCreateWithFlags(&ev_fork_, hipEventDisableTiming));
        sc_half_.alloc((size_t)parts * nsub);
        // deal the members into parts of equal fine-level work (largest first, to the lightest
        // part; the lower part index on ties)
        std::vector<int> ord(nsub);
        for (int s = 0; s < nsub; ++s) ord[s] = s;
        std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return lev.back().nnzb_sub[x] > lev.back().nnzb_sub[y]; });
        half_host_.assign(nsub, 0);
        double w[kMaxParts] = {0.0, 0.0, 0.0, 0.0};
        for (int s : ord) {
            int h = 0;
            for (int q = 1; q < parts; ++q)
                if (w[q] < w[h]) h = q;
            half_host_[s] = h;
            w[h] += (double)lev.back().nnzb_sub[s];
        }
        half_.upload(half_host_);
    }
    split_ = on;
}

// Host pacing of the parts' replays (pace_until_done per part, one loop): a part gets its next
// replay when its slowest member has entered the last one enqueued for it.
int64_t pace_parts(int np, hipStream_t* st, hipGraphExec_t* g, const MirrorBuf& m, const std::vector<int>& part, int64_t k,
                   int64_t launched0, hipGraphExec_t* g1, const int64_t* horizon) {
    constexpr int64_t kRunway = 2;
    if (np < 1 || np > kMaxParts) throw ApiError(DDPCA_EINVAL, "pace_parts: part count");
    int64_t launched[kMaxParts], replays = 0;
    for (int h = 0; h < np; ++h) launched[h] = launched0;
    for (int64_t spin = 0;; ++spin) {
        bool all = true;
        int64_t slowest[kMaxParts];
        bool busy[kMaxParts], tail[kMaxParts];
        for (int h = 0; h < np; ++h) slowest[h] = INT64_MAX, busy[h] = false;
        for (int s = 0; s < m.n; ++s) {
            if (__atomic_load_n(&m.host[s].done, __ATOMIC_ACQUIRE)) continue;
            all = false;
            busy[part[s]] = true;
            slowest[part[s]] = std::min<int64_t>(slowest[part[s]], __atomic_load_n(&m.host[s].iter, __ATOMIC_RELAXED));
        }
        if (all) return replays;
        bool launched_now = false;
        for (int h = 0; h < np; ++h) {
            tail[h] = g1 && horizon && g1[h] && launched[h] + k > horizon[h];
            if (busy[h] && (tail[h] ? launched[h] - slowest[h] <= kRunway : launched[h] - slowest[h] <= k)) {
                DDPCA_HIP(hipGraphLaunch(tail[h] ? g1[h] : g[h], st[h]));
                launched[h] += tail[h] ? 1 : k;
                ++replays;
                launched_now = true;
            }
        }
        if (launched_now) continue;
        if ((spin & 255) == 255) {
            for (int h = 0; h < np; ++h) {
                if (!busy[h]) continue;
                const hipError_t q = hipStreamQuery(st[h]);
                if (q == hipSuccess) {
                    // this part's stream drained: its mirror entries are final for what it ran
                    bool done_now = true;
                    for (int s = 0; s < m.n; ++s)
                        if (part[s] == h) done_now &= __atomic_load_n(&m.host[s].done, __ATOMIC_ACQUIRE) != 0;
                    if (!done_now) {
                        DDPCA_HIP(hipGraphLaunch(tail[h] ? g1[h] : g[h], st[h]));
                        launched[h] += tail[h] ? 1 : k;
                        ++replays;
                    }
                } else if (q != hipErrorNotReady) {
                    DDPCA_HIP(q);
                }
            }
        }
        std::this_thread::yield();
    }
}

void MgpisDevice::pcg_begin(int prec, double rtol, const std::vector<int64_t>& maxit, bool warm) {
    select_device(device);
    last_prec_ = prec;
    solve_accounted_ = prec != 1 || warm;  // the byte model covers the V-cycle PCG from x0 = 0
    if ((int)maxit.size() != nsub) throw ApiError(DDPCA_EINVAL, "maxit per subdomain");
    build_graph(prec);
    LevelDev& L = lev.back();
    // the previous solve on this stream has finished (pcg_finish synchronised), so the
    // host-side reset of the mirror and the staging buffer cannot race a kernel
    mirror.reset();
    for (int s = 0; s < nsub; ++s) {
        sc_host[s] = PcgScal{};
        sc_host[s].tol2 = rtol * rtol;
        sc_host[s].maxit = maxit[s];
    }
    DDPCA_HIP(hipMemcpyAsync(sc.p, sc_host, nsub * sizeof(PcgScal), hipMemcpyHostToDevice, stream));
    const int nblk = ceil_div(L.nn, kBlock);
    if (!warm) {
        hipLaunchKernelGGL(k_pcg_init, dim3(nblk), dim3(kBlock), 0, stream, bs.p, xs.p, rs.p, ps.p, qs.p, partial.p, L.nn);
        launch_fin(stream, (int)kFinInit, partial.p, nullptr, fin_cb.p, sc.p, mirror.dev);
    } else {
        double* partial2 = partial.p + L.nch;
        hipLaunchKernelGGL(k_pcg_init_warm, dim3(nblk), dim3(kBlock), 0, stream, bs.p, ps.p, qs.p, partial2, L.nn);
        SellArgs a = level_args(L);
        a.x = xs.p;
        a.b = bs.p;
        a.y = rs.p;
        a.partial = partial.p;
        launch_sell<kResid, false, true>(kVal64, a, stream);
        launch_fin(stream, (int)kFinInitWarm, partial.p, partial2, fin_cb.p, sc.p, mirror.dev);
    }
    if (prec == 1) vcycle(rs.p, zs.p, true);
    else hipLaunchKernelGGL(k_diag, dim3(nblk), dim3(kBlock), 0, stream, rs.p, L.dinv.p, zs.p, partial.p, L.nn, L.csub.p, sc.p);
    launch_fin(stream, (int)kFinBeta0, prec == 1 ? vc_partial() : partial.p, nullptr, prec == 1 ? vc_cb() : fin_cb.p, sc.p,
               mirror.dev);
    sample_pending_ = false;
    if (time_kernel) {
        // first iteration eagerly, with HIP events around its fine-level SpMV on this stream
        enqueue_iteration(prec, true);
        sample_pending_ = true;
    }
    if (split_) {
        // fork: each half continues on its own stream from its own copy of the scalars
        hipLaunchKernelGGL(k_split_sc, dim3(ceil_div(nsub, 64)), dim3(64), 0, stream, sc.p, sc_half_.p, half_.p, nsub,
                           nparts_);
        DDPCA_HIP(hipEventRecord(ev_fork_, stream));
        for (int h = 1; h < nparts_; ++h) DDPCA_HIP(hipStreamWaitEvent(part_stream(h), ev_fork_, 0));
    }
}

void MgpisDevice::pcg_step(int prec) {
    if (split_) {
        for (int h = 0; h < nparts_; ++h) DDPCA_HIP(hipGraphLaunch(graph_h_[prec][h], part_stream(h)));
        graphs_launched += nparts_;
        return;
    }
    DDPCA_HIP(hipGraphLaunch(graph_[prec], stream));
    ++graphs_launched;
}

void MgpisDevice::pcg_wait(int prec, int64_t pre_enqueued) {
    const int64_t k = opt.iters_per_graph;
    const int64_t launched = (sample_pending_ ? 1 : 0) + pre_enqueued * k;
    if (split_) {
        hipStream_t st[kMaxParts];
        int64_t hz[kMaxParts];
        for (int h = 0; h < nparts_; ++h) st[h] = part_stream(h), hz[h] = horizon(prec, h);
        graphs_launched += pace_parts(nparts_, st, graph_h_[prec], mirror, half_host_, k, launched, graph1_h_[prec], hz);
        // join: `stream` continues after the other parts' replays; the scalars merge back
        for (int h = 1; h < nparts_; ++h) {
            DDPCA_HIP(hipEventRecord(ev_join_[h - 1], part_stream(h)));
            DDPCA_HIP(hipStreamWaitEvent(stream, ev_join_[h - 1], 0));
        }
        hipLaunchKernelGGL(k_merge_sc, dim3(ceil_div(nsub, 64)), dim3(64), 0, stream, sc.p, sc_half_.p, half_.p, nsub);
        return;
    }
    graphs_launched += pace_until_done(stream, graph_[prec], mirror, k, launched, graph1_[prec], horizon(prec, -1));
}

void MgpisDevice::pcg_fetch() {
    DDPCA_HIP(hipMemcpyAsync(sc_host, sc.p, nsub * sizeof(PcgScal), hipMemcpyDeviceToHost, stream));
}

void MgpisDevice::pcg_finish() {
    pcg_fetch();
    DDPCA_HIP(hipStreamSynchronize(stream));
    pcg_check();
}

void MgpisDevice::pcg_check() {
    if (sample_pending_) {
        // the sampled launch did work only for members that ran an iteration (the others were
        // done at init, e.g. zero right-hand side, and their chunks exited at once)
        double bytes = 0.0;
        for (int s = 0; s < nsub; ++s)
            if (sc_host[s].iter >= 1) bytes += fine_kernel_bytes(s);
        float ms = 0.f;
        if (bytes > 0.0 && hipEventElapsedTime(&ms, ev_k0, ev_k1) == hipSuccess && ms > 0.f) {
            timed_kernel_ms += ms;
            timed_kernel_bytes += bytes;
            timed_kernel_samples += 1;
        }
        sample_pending_ = false;
    }
    for (int s = 0; s < nsub; ++s)
        if (sc_host[s].fail) throw ApiError(DDPCA_ENUMERIC, "PCG breakdown (non-finite or non-positive curvature) in batch member " + std::to_string(s));
    // this solve's iteration counts pace the next one's tail (pcg_wait)
    if (last_prec_ >= 0) {
        expect_[last_prec_].resize(nsub);
        for (int s = 0; s < nsub; ++s) expect_[last_prec_][s] = sc_host[s].iter;
        last_prec_ = -1;
    }
    if (!no_coarse && !solve_accounted_) {
        // algorithmic bytes of the solve that just finished: members done at initialisation moved
        // only k_pcg_init's share; the others ran iter SpMVs and iter V-cycles (the setup's
        // first one and iter - 1 more: the converging iteration skips its V-cycle)
        for (int s = 0; s < nsub; ++s) {
            const double n = (double)lev.back().nloc[s];
            if (sc_host[s].iter == 0) {
                alg_bytes[0] += 120.0 * n;
                continue;
            }
            double a[2], b[2];
            setup_bytes(s, a);
            iteration_bytes(s, b);
            double v[2];
            vcycle_bytes(s, v);
            const double it = (double)sc_host[s].iter;
            alg_bytes[0] += a[0] + it * b[0] - v[0];
            alg_bytes[1] += a[1] + it * b[1] - v[1];
        }
        int64_t itmax = 0;
        for (int s = 0; s < nsub; ++s) itmax = std::max<int64_t>(itmax, sc_host[s].iter);
        alg_bytes[2] += (double)(itmax * iteration_launches());
        solve_accounted_ = true;
    }
}

void MgpisDevice::pcg_solve(int prec, double rtol, const std::vector<int64_t>& maxit, bool warm) {
    pcg_begin(prec, rtol, maxit, warm);
    pcg_wait(prec, 0);
    pcg_finish();
}

void MgpisDevice::scatter_free(int s, const double* cond, double* full) {
    DDPCA_HIP(hipMemsetAsync(full + 3 * lev.back().noff[s], 0, 3 * pad64(lev.back().nloc[s]) * sizeof(double), stream));
    hipLaunchKernelGGL(k_scatter, dim3(ceil_div(nfree[s], kBlock)), dim3(kBlock), 0, stream, cond, free_dof[s].p, full, nfree[s]);
}

void MgpisDevice::gather_free(int s, const double* full, double* cond) {
    hipLaunchKernelGGL(k_gather, dim3(ceil_div(nfree[s], kBlock)), dim3(kBlock), 0, stream, full, free_dof[s].p, cond, nfree[s]);
}

}  // namespace ddpca
