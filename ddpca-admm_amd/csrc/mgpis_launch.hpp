// Launch interface between the device_mgpis*.hip sources: the argument structs of the SELL and
// colour-sweep kernels, the mode enums, the dispatch from run-time storage choices to C++ types,
// and the host entry points one file offers the others.  Internal to those sources.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "device_mgpis.hpp"

namespace ddpca {

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

// ---- host entry points across the files
// Krylov-operator arguments (fp64 values) of a level (device_mgpis.hip)
SellArgs level_args(const LevelDev& L);
// one SELL launch over a level: table mode when the arguments carry a table, else values streamed
// in storage type vt (device_mgpis.hip; beyond that file's own uses, instantiated for the PCG's
// <kPcg, false, true> and <kResid, false, true>)
template <int MODE, bool BJ, bool DOT>
void launch_sell(int vt, const SellArgs& a, hipStream_t s);
// one colour-sweep launch: phase PH over the chunks k selects (device_mgpis_gs.hip; instantiated
// for the <PH, DOT> pairs vcycle() issues)
template <int PH, bool DOT>
void launch_gs(const MgpisDevice& D, int k, double* x, const double* b, double* r, const PcgScal* scp, double* partial);

}  // namespace ddpca
