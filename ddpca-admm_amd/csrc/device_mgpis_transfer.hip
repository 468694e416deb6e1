// MGPIS device path: the V-cycle's grid transfers, the first sweep from a zero guess and the dense
// coarse solve, with the MgpisDevice methods that launch them (node-parallel kernels, thread =
// node: NODE_PROLOGUE, mgpis_device_fn.hpp).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "device_mgpis.hpp"
#include "mgpis_device_fn.hpp"
#include "mgpis_launch.hpp"

namespace ddpca {

namespace {

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
    const double s = wsum(s0 + s1);
    if (lane == 0) x[r] = s;
}

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

}  // namespace ddpca
