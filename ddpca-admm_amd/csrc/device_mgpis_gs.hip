// MGPIS device path: the fine level's multicolour sweeps (GsFine, device_mgpis.hpp) -- colour
// Gauss-Seidel, colour SSOR and the band mode's ring / far rows -- and their one launcher.
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include "device_mgpis.hpp"
#include "mgpis_device_fn.hpp"
#include "mgpis_launch.hpp"

namespace ddpca {

namespace {

// (GsArgs, the sweeps' arguments with the phases of k_gs: mgpis_launch.hpp)

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

// the colour copy the sweeps stream: its storage type and values (GsFine holds exactly one)
std::pair<int, const void*> gs_values(const GsFine& G) {
    if (G.val8.p) return {kValQ8, G.val8.p};
    if (G.val16.p) return {kValH16, G.val16.p};
    if (G.val32.p) return {kVal32, G.val32.p};
    return {kVal64, G.val64.p};
}
}  // namespace

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
            if constexpr (PH >= 6) {  // (the fp64 copy was refused above)
                if constexpr (!std::is_same_v<T, double>) {
                    if (a.x4) hipLaunchKernelGGL((k_gs_ssor<PH, DOT, T, CT, true>), grid, dim3(kWave), 0, D.stream, a);
                    else hipLaunchKernelGGL((k_gs_ssor<PH, DOT, T, CT>), grid, dim3(kWave), 0, D.stream, a);
                }
            } else if constexpr (PH >= 3) {  // the band mode's ring / far groups
                hipLaunchKernelGGL((k_gs_aux<PH, T, CT>), grid, dim3(kWave), 0, D.stream, a);
            } else {
                if (a.x4) hipLaunchKernelGGL((k_gs<PH, DOT, T, CT, true>), grid, dim3(kWave), 0, D.stream, a);
                else hipLaunchKernelGGL((k_gs<PH, DOT, T, CT>), grid, dim3(kWave), 0, D.stream, a);
            }
        });
    });
}

// the launches vcycle() issues: Gauss-Seidel 0 / 1 / 2, the band's 3 / 4 / 5, SSOR 6 .. 10; the
// dot product's partials come with the last backward sweep only
template void launch_gs<0, false>(const MgpisDevice&, int, double*, const double*, double*, const PcgScal*, double*);
template void launch_gs<1, false>(const MgpisDevice&, int, double*, const double*, double*, const PcgScal*, double*);
template void launch_gs<2, false>(const MgpisDevice&, int, double*, const double*, double*, const PcgScal*, double*);
template void launch_gs<2, true>(const MgpisDevice&, int, double*, const double*, double*, const PcgScal*, double*);
template void launch_gs<3, false>(const MgpisDevice&, int, double*, const double*, double*, const PcgScal*, double*);
template void launch_gs<4, false>(const MgpisDevice&, int, double*, const double*, double*, const PcgScal*, double*);
template void launch_gs<5, false>(const MgpisDevice&, int, double*, const double*, double*, const PcgScal*, double*);
template void launch_gs<6, false>(const MgpisDevice&, int, double*, const double*, double*, const PcgScal*, double*);
template void launch_gs<7, false>(const MgpisDevice&, int, double*, const double*, double*, const PcgScal*, double*);
template void launch_gs<8, false>(const MgpisDevice&, int, double*, const double*, double*, const PcgScal*, double*);
template void launch_gs<9, false>(const MgpisDevice&, int, double*, const double*, double*, const PcgScal*, double*);
template void launch_gs<10, false>(const MgpisDevice&, int, double*, const double*, double*, const PcgScal*, double*);
template void launch_gs<10, true>(const MgpisDevice&, int, double*, const double*, double*, const PcgScal*, double*);

}  // namespace ddpca
