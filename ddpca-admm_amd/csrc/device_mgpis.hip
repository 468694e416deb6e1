// MGPIS device path: the SELL-BSR3 kernels with their dispatch and the V-cycle for gfx950 over a
// batch of subdomains (see device_mgpis.hpp for the layout).  The colour sweeps, the grid
// transfers, the PCG recurrence and the setup are device_mgpis_{gs,transfer,pcg,setup}.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "device_mgpis.hpp"
#include "mgpis_device_fn.hpp"
#include "mgpis_launch.hpp"

namespace ddpca {

// ============================================================================== kernels
namespace {

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

// partial x^T y per chunk (used after a coarse-only "V-cycle")
__global__ __launch_bounds__(kBlock) void k_dot(const double* x, const double* y, double* partial, int64_t nn,
                                                const int32_t* csub, const PcgScal* sc) {
    NODE_PROLOGUE(nn, csub, sc)
    double s = 0.0;
    for (int a = 0; a < 3; ++a) s += x[3 * i + a] * y[3 * i + a];
    chunk_partial(s, partial, i >> 6);
}
}  // namespace

// ============================================================================== operations
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
// the PCG's launches (device_mgpis_pcg.hip): the iteration's SpMV and the warm start's residual
template void launch_sell<kPcg, false, true>(int, const SellArgs&, hipStream_t);
template void launch_sell<kResid, false, true>(int, const SellArgs&, hipStream_t);

namespace {
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

}  // namespace ddpca
