// Batched surface-mass solver (device_mass.hpp): kernels and MassBatch's member definitions.
#include "device_mass.hpp"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "../../include/ddpca_amd.h"

namespace ddpca {

namespace {

// ---- batched Jacobi-PCG over the owned sides' surface mass systems.  Rows of all systems
// are concatenated, each padded to a multiple of 64 (ELL-64: chunk = 64 rows = one wave,
// lane = row, slot k at (off[c]+k)*64 + lane); per-system scalars live in PcgScal.
struct EllArgs {
    const int32_t* slots;
    const int64_t* off;
    const int32_t* col;
    const double* val;
    const int32_t* csys;
    const double* dinv;
    int64_t nch;
};

// r = b, x = 0, z = D^-1 b, p = q = 0; partials (b.z, b.b) per chunk
__global__ __launch_bounds__(256) void k_mcg_init(const double* b, const double* dinv, double* x, double* r, double* z,
                                                  double* p, double* q, double* partial, int64_t nrow) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nrow) return;
    const double bi = b[i], zi = dinv[i] * bi;
    x[i] = 0.0;
    r[i] = bi;
    z[i] = zi;
    p[i] = 0.0;
    q[i] = 0.0;
    const double a = wsum(bi * zi), c = wsum(bi * bi);
    if ((threadIdx.x & 63) == 0) {
        partial[2 * (i >> 6)] = a;
        partial[2 * (i >> 6) + 1] = c;
    }
}

// q = A z + beta q, p = z + beta p; partial p.q per chunk (at partial[ostride * chunk]).  The paired
// form runs over a batch whose second half repeats the first half's matrices R rows further on
// (MassBatch::paired_; the fused w|v interface update: both sides' v systems carry the w systems'
// inteMass): a wave takes chunk c and its twin c + nch_launch, reads the stored entries once and
// gathers z at j and j + R.  Each row's sum runs over the same slots in the same order in both
// forms, so q, p and the partials are bit for bit the same; the matrix stream is halved.
template <bool PAIR>
__global__ __launch_bounds__(256) void k_mcg_spmv(EllArgs e, const PcgScal* sc, const double* z, double* q, double* p,
                                                  double* partial, int ostride, int64_t R, int64_t nch_launch) {
    const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= nch_launch) return;
    const int sw = e.csys[c];
    const int sv = PAIR ? e.csys[c + nch_launch] : sw;
    const bool aw = !sc[sw].done, av = PAIR && !sc[sv].done;
    if (!aw && !av) return;
    const int lane = threadIdx.x & 63;
    const int64_t row = c * 64 + lane;
    const int ns = e.slots[c];
    const int32_t* cp = e.col + e.off[c] * 64 + lane;
    const double* vp = e.val + e.off[c] * 64 + lane;
    double s0 = 0.0, s1 = 0.0;
#pragma unroll 4
    for (int k = 0; k < ns; ++k) {
        const double v = vp[(int64_t)k * 64];
        const int32_t j = cp[(int64_t)k * 64];
        s0 += v * z[j];
        if (PAIR) s1 += v * z[j + R];
    }
    auto upd = [&](int sys, int64_t i, int64_t chunk, double sum) {
        const double be = sc[sys].beta;
        const double qi = sum + be * q[i], pi = z[i] + be * p[i];
        q[i] = qi;
        p[i] = pi;
        const double d = wsum(pi * qi);
        if (lane == 0) partial[ostride * chunk] = d;
    };
    if (aw) upd(sw, row, c, s0);
    if (av) upd(sv, row + R, c + nch_launch, s1);
}

// x += alpha p, r -= alpha q, z = D^-1 r; partials (r.r, r.z) per chunk: the update of row i, shared
// by the two forms of the step length below
__device__ __forceinline__ void mcg_update(double al, int64_t i, const double* dinv, double* x, double* r, double* z,
                                           const double* p, const double* q, double* partial) {
    x[i] += al * p[i];
    const double ri = r[i] - al * q[i], zi = dinv[i] * ri;
    r[i] = ri;
    z[i] = zi;
    const double a = wsum(ri * ri), b = wsum(ri * zi);
    if ((threadIdx.x & 63) == 0) {
        partial[2 * (i >> 6)] = a;
        partial[2 * (i >> 6) + 1] = b;
    }
}

// the update with alpha computed in place of a k_mcg_fin(kMcgAlpha) launch: every wave sums its
// system's p.q chunk partials (ppq, written by k_mcg_spmv with stride 1 -- not the (r.r, r.z)
// pairs this kernel writes) in one fixed order, so all waves hold the same alpha; the system's
// first chunk stores alpha / p.q and the breakdown flag as k_mcg_fin does.  On a breakdown (p.q
// not positive or not finite) every wave sees the same p.q and leaves x, r, z untouched, so x
// keeps the last good iterate as with the separate k_mcg_fin launch.  Every wave re-reads its
// system's partials (chunks^2 L2 reads per system), so MassBatch takes this form only up to
// kMcgFuseMaxChunks chunks (65,536 rows) per system; the headline's sides have up to ~300.
constexpr int64_t kMcgFuseMaxChunks = 1024;
__global__ __launch_bounds__(256) void k_mcg_axpy_fa(EllArgs e, PcgScal* sc, double* x, double* r, double* z,
                                                     const double* p, const double* q, double* partial,
                                                     const double* ppq, const int64_t* cb, PcgMirror* mirror) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t c = i >> 6;
    if (c >= e.nch) return;
    const int sys = e.csys[c];
    if (sc[sys].done) return;
    const int lane = threadIdx.x & 63;
    double pq = 0.0;
    for (int64_t k = cb[sys] + lane; k < cb[sys + 1]; k += 64) pq += ppq[k];
    pq = wsum(pq);
    const double al = sc[sys].delta / pq;
    const bool bad = !(pq > 0.0) || !isfinite(pq);  // the same in every wave of the system
    if (c == cb[sys] && lane == 0) {
        sc[sys].pq = pq;
        sc[sys].alpha = al;
        if (bad) {
            sc[sys].fail = 1;
            sc[sys].done = 1;
            mirror_store(mirror + sys, sc[sys].iter, 1, 1);
        }
    }
    if (bad) return;
    mcg_update(al, i, e.dinv, x, r, z, p, q, partial);
}

// the update with alpha from k_mcg_fin(kMcgAlpha)
__global__ __launch_bounds__(256) void k_mcg_axpy(EllArgs e, const PcgScal* sc, double* x, double* r, double* z,
                                                  const double* p, const double* q, double* partial) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t c = i >> 6;
    if (c >= e.nch) return;
    const int sys = e.csys[c];
    if (sc[sys].done) return;
    mcg_update(sc[sys].alpha, i, e.dinv, x, r, z, p, q, partial);
}

// ---- Chebyshev iteration on D^-1 M (MassBatch::cheb_; Saad, Iterative Methods, Alg. 12.1): a fixed
// number of steps from setup bounds of each system's spectrum, one launch per step, no reductions;
// the CG below then restarts from its iterate (k_mcg_restart) and usually finds it converged.
// x = 0, r = b, d = D^-1 b / theta_sys
__global__ __launch_bounds__(256) void k_mcheb_init(const double* b, const double* dinv, const double* ith,
                                                    const int32_t* csys, double* x, double* r, double* d, int64_t nrow) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nrow) return;
    const double bi = b[i];
    x[i] = 0.0;
    r[i] = bi;
    d[i] = ith[csys[i >> 6]] * dinv[i] * bi;
}

// step k: x += d, r -= M d, dn = c1 d + c2 D^-1 r (coef[(k nsys + sys) 2 + {0, 1}]); systems whose
// step count kmax is reached keep their x, r.  The paired form (MassBatch::paired_) reads the
// shared matrix once for chunk c and its twin c + nch_launch, as k_mcg_spmv<true>.
template <bool PAIR>
__global__ __launch_bounds__(256) void k_mcheb_step(EllArgs e, const double* coef, const int32_t* kmax, int nsys, int k,
                                                    const double* d, double* dn, double* x, double* r, int64_t R,
                                                    int64_t nch_launch) {
    const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= nch_launch) return;
    const int sw = e.csys[c];
    const int sv = PAIR ? e.csys[c + nch_launch] : sw;
    const bool aw = k < kmax[sw], av = PAIR && k < kmax[sv];
    if (!aw && !av) return;
    const int lane = threadIdx.x & 63;
    const int64_t row = c * 64 + lane;
    const int ns = e.slots[c];
    const int32_t* cp = e.col + e.off[c] * 64 + lane;
    const double* vp = e.val + e.off[c] * 64 + lane;
    double s0 = 0.0, s1 = 0.0;
#pragma unroll 4
    for (int q = 0; q < ns; ++q) {
        const double v = vp[(int64_t)q * 64];
        const int32_t j = cp[(int64_t)q * 64];
        s0 += v * d[j];
        if (PAIR) s1 += v * d[j + R];
    }
    auto upd = [&](int sys, int64_t i, double sum) {
        const double di = d[i];
        x[i] += di;
        const double ri = r[i] - sum;
        r[i] = ri;
        const double* cc = coef + 2 * ((int64_t)k * nsys + sys);
        dn[i] = cc[0] * di + cc[1] * e.dinv[i] * ri;
    };
    if (aw) upd(sw, row, s0);
    if (av) upd(sv, row + R, s1);
}

// The matrix kernels' launch shape: f(PAIR as a type, R, chunks of the launch) -- a paired launch
// covers the first half's chunks, R = nrow / 2 rows from their twins
template <typename F>
void with_pairing(bool pair, int64_t nrow, int64_t nch, F&& f) {
    if (pair) f(std::true_type{}, nrow / 2, nch / 2);
    else f(std::false_type{}, (int64_t)0, nch);
}

// CG restart from the Chebyshev iterate: z = D^-1 r, p = q = 0; partials (r.z, r.r) per chunk and
// b.b per chunk at bb (the stop rule stays relative to ||b||)
__global__ __launch_bounds__(256) void k_mcg_restart(const double* b, const double* dinv, const double* r, double* z,
                                                     double* p, double* q, double* partial, double* bbp, int64_t nrow) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nrow) return;
    const double ri = r[i], zi = dinv[i] * ri, bi = b[i];
    z[i] = zi;
    p[i] = 0.0;
    q[i] = 0.0;
    const double a = wsum(ri * zi), c = wsum(ri * ri), d = wsum(bi * bi);
    if ((threadIdx.x & 63) == 0) {
        partial[2 * (i >> 6)] = a;
        partial[2 * (i >> 6) + 1] = c;
        bbp[i >> 6] = d;
    }
}

enum McgWhat { kMcgInit = 0, kMcgAlpha = 1, kMcgBeta = 2 };

// the CG's scalars at its start: delta = r.z, rr = r.r, bb = b.b, tol2 scaled by b.b
__device__ __forceinline__ void mcg_scal_start(PcgScal* sc, double delta, double rr, double bb) {
    sc->delta = delta;
    sc->bb = bb;
    sc->rr = rr;
    sc->tol2 = sc->tol2 * bb;
    sc->beta = 0.0;
    sc->iter = 0;
    sc->fail = 0;
    sc->done = (rr <= sc->tol2 || sc->maxit <= 0) ? 1 : 0;
}

// per-system scalars: one workgroup per system, fixed order over its chunks
__global__ __launch_bounds__(256) void k_mcg_fin(int what, const double* partial, const int64_t* cb, PcgScal* scv,
                                                 PcgMirror* mirror) {
    const int sys = blockIdx.x;
    PcgScal* sc = scv + sys;
    if (what != kMcgInit && sc->done) return;
    __shared__ double r0[4], r1[4];
    // four independent accumulator pairs per thread (loads in flight together), fixed order
    double av[4] = {0.0, 0.0, 0.0, 0.0}, bv[4] = {0.0, 0.0, 0.0, 0.0};
    const int64_t k1 = cb[sys + 1];
    for (int64_t k = cb[sys] + threadIdx.x; k < k1; k += 4 * 256) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t q = k + 256 * u;
            if (q < k1) {
                av[u] += partial[2 * q];
                bv[u] += partial[2 * q + 1];
            }
        }
    }
    double a = wsum((av[0] + av[1]) + (av[2] + av[3]));
    double b = wsum((bv[0] + bv[1]) + (bv[2] + bv[3]));
    if ((threadIdx.x & 63) == 0) {
        r0[threadIdx.x >> 6] = a;
        r1[threadIdx.x >> 6] = b;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    a = (r0[0] + r0[1]) + (r0[2] + r0[3]);
    b = (r1[0] + r1[1]) + (r1[2] + r1[3]);
    if (what == kMcgInit) {
        // x0 = 0: ||r0||^2 = b.b
        mcg_scal_start(sc, a, b, b);
        mirror_store(mirror + sys, 0, sc->done, 0);
    } else if (what == kMcgAlpha) {
        sc->pq = a;
        if (!(a > 0.0) || !isfinite(a)) {
            sc->fail = 1;
            sc->done = 1;
            mirror_store(mirror + sys, sc->iter, 1, 1);
        }
        sc->alpha = sc->delta / a;
    } else {
        sc->rr = a;
        sc->iter += 1;
        if (!isfinite(a) || !isfinite(b)) sc->fail = 1;
        if (sc->fail || a <= sc->tol2 || sc->iter >= sc->maxit) sc->done = 1;
        sc->beta = b / sc->delta;
        sc->delta = b;
        mirror_store(mirror + sys, sc->iter, sc->done, sc->fail);
    }
}

// the CG's scalars after k_mcg_restart: delta = r.z, rr = r.r, bb = b.b (one workgroup per system,
// a fixed order), as k_mcg_fin's init sets them
__global__ __launch_bounds__(256) void k_mcg_fin_restart(const double* partial, const double* bbp, const int64_t* cb,
                                                         PcgScal* scv, PcgMirror* mirror) {
    const int sys = blockIdx.x;
    PcgScal* sc = scv + sys;
    __shared__ double r0[4], r1[4], r2[4];
    double a = 0.0, b = 0.0, c = 0.0;
    for (int64_t k = cb[sys] + threadIdx.x; k < cb[sys + 1]; k += 256) {
        a += partial[2 * k];
        b += partial[2 * k + 1];
        c += bbp[k];
    }
    a = wsum(a);
    b = wsum(b);
    c = wsum(c);
    if ((threadIdx.x & 63) == 0) {
        r0[threadIdx.x >> 6] = a;
        r1[threadIdx.x >> 6] = b;
        r2[threadIdx.x >> 6] = c;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    a = (r0[0] + r0[1]) + (r0[2] + r0[3]);
    b = (r1[0] + r1[1]) + (r1[2] + r1[3]);
    c = (r2[0] + r2[1]) + (r2[2] + r2[3]);
    mcg_scal_start(sc, a, b, c);
    if (!(c > 0.0)) sc->done = 1;
    if (!isfinite(a) || !isfinite(b)) {
        sc->fail = 1;
        sc->done = 1;
    }
    mirror_store(mirror + sys, 0, sc->done, sc->fail);
}

// scs[h][i] = sc[i] with done forced on the other half's systems / sc[i] = its half's copy
__global__ void k_scal_split(const PcgScal* sc, PcgScal* scs, const int32_t* half, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int h = 0; h < 2; ++h) {
        PcgScal v = sc[i];
        if (half[i] != h) v.done = 1;
        scs[h * n + i] = v;
    }
}
__global__ void k_scal_merge(PcgScal* sc, const PcgScal* scs, const int32_t* half, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sc[i] = scs[half[i] * n + i];
}

}  // namespace

void MassBatch::build(const std::vector<const Csr*>& A, const std::vector<int64_t>& roff, int64_t nrow_total) {
    nsys = (int)A.size();
    nrow = nrow_total;
    nch = nrow / 64;
    // DDPCA_MASS_CHEB=0 keeps the plain CG
    const char* ce = std::getenv("DDPCA_MASS_CHEB");
    MassPlan P = mass_plan(A, roff, nrow, !(ce && ce[0] == '0'));
    paired_ = P.paired;
    slots.upload(P.slots);
    csys.upload(P.csys);
    off.upload(P.off);
    col.upload(P.col);
    val.upload(P.val);
    dinv.upload(P.dinv);
    cb.upload(P.cb);
    cb_host_ = P.cb;
    // algorithmic bytes per system: init (b, D^-1 read; x r z p q written: 56 B per row) and
    // per CG iteration -- k_mcg_spmv: stored entries (12 B), z gathered once, z, q, p read
    // and q, p written; k_mcg_axpy: x, r read + written, z written, p, q, D^-1 read (112 B per row)
    init_bytes_.assign(nsys, 0.0);
    it_bytes_.assign(nsys, 0.0);
    mat_bytes_.assign(nsys, 0.0);
    for (int s = 0; s < nsys; ++s) {
        const double rows = (double)A[s]->nrow, ent = (double)A[s]->nnz();
        init_bytes_[s] = 56.0 * rows;
        // (+ the p.q and (r.r, r.z) chunk partials written once and read once: 24 B each way per chunk)
        it_bytes_[s] = 8.0 * rows + 40.0 * rows + 64.0 * rows + 48.0 * (double)(pad64(A[s]->nrow) / 64);
        mat_bytes_[s] = 12.0 * ent;  // (paired: once per pair, for the pair's longer solve)
    }
    for (auto* v : {&b, &x, &r, &z, &p, &q}) {
        v->alloc(std::max<int64_t>(nrow, 2));
        v->zero();
    }
    partial.alloc(3 * std::max<int64_t>(nch, 1));  // (a, b) pairs + the fused form's p.q
    sc.alloc(std::max(nsys, 1));
    cheb_ = P.cheb;
    lam_lo_ = P.lam_lo;
    lam_hi_ = P.lam_hi;
    // the ADMM loop's tolerance planned here, at setup: solve() uploads nothing while other
    // in-process ranks may be capturing graphs
    if (cheb_) plan_cheb(1.0e-14);
    DDPCA_HIP(hipHostMalloc(reinterpret_cast<void**>(&sc_host), std::max(nsys, 1) * sizeof(PcgScal)));
    mirror.alloc(nsys);
}

MassBatch::~MassBatch() {
    if (s2_) (void)hipStreamSynchronize(s2_);
    drop_graphs();
    if (ev_fork_) (void)hipEventDestroy(ev_fork_);
    if (ev_join_) (void)hipEventDestroy(ev_join_);
    if (s2_) (void)hipStreamDestroy(s2_);
    if (sc_host) (void)hipHostFree(sc_host);
}

void MassBatch::solve(hipStream_t s, double* x_out, double rtol, int64_t maxit) {
    if (nsys == 0) return;
    solved_ = true;
    if (x_out != x_target_) {
        drop_graphs();
        x_target_ = x_out;
    }
    if (cheb_ && rtol != cheb_rtol_) {
        // a tolerance other than the setup plan's (1e-14, the ADMM loop's): re-plan and
        // re-capture here -- the capture holds the library's capture lock (device_common.hpp)
        drop_graphs();
        plan_cheb(rtol);
    }
    if (!graph_) capture(s);
    mirror.reset();  // the previous solve on `s` was paced to completion before this point
    for (int i = 0; i < nsys; ++i) {
        sc_host[i] = PcgScal{};
        sc_host[i].tol2 = rtol * rtol;
        sc_host[i].maxit = maxit;
    }
    DDPCA_HIP(hipMemcpyAsync(sc.p, sc_host, nsys * sizeof(PcgScal), hipMemcpyHostToDevice, s));
    // Chebyshev mode: the fixed-length Chebyshev graph, then the CG restarted from its iterate
    // (the host launches CG replays only once the mirror says a system is not done, or the
    // stream drained); else x0 = 0 (warm starts from the previous ADMM iteration's solution:
    // 39.3 -> 37.1 mass-CG iterations at the headline, no measurable gain, profiles/r03v)
    int64_t launched0 = 0;
    cheb_used_ = cheb_ && cgraph_;
    if (cheb_used_) {
        DDPCA_HIP(hipGraphLaunch(cgraph_, s));
        launched0 = k + 1;
    } else {
        hipLaunchKernelGGL(k_mcg_init, dim3(nb256(nrow)), dim3(256), 0, s, b.p, dinv.p, x_out, r.p, z.p, p.p, q.p,
                           partial.p, nrow);
        hipLaunchKernelGGL(k_mcg_fin, dim3(nsys), dim3(256), 0, s, (int)kMcgInit, partial.p, cb.p, sc.p, mirror.dev);
    }
    if (split_) {
        // fork into the two halves' streams, pace both, join and merge the scalars back
        hipLaunchKernelGGL(k_scal_split, dim3(ceil_div(nsys, 64)), dim3(64), 0, s, sc.p, sc_half_.p, half_.p, nsys);
        DDPCA_HIP(hipEventRecord(ev_fork_, s));
        DDPCA_HIP(hipStreamWaitEvent(s2_, ev_fork_, 0));
        hipStream_t st[2] = {s, s2_};
        const int64_t hz[2] = {horizon(0), horizon(1)};
        pace_halves(st, graph_h_, mirror, half_host_, k, launched0, graph1_h_, hz);
        DDPCA_HIP(hipEventRecord(ev_join_, s2_));
        DDPCA_HIP(hipStreamWaitEvent(s, ev_join_, 0));
        hipLaunchKernelGGL(k_scal_merge, dim3(ceil_div(nsys, 64)), dim3(64), 0, s, sc.p, sc_half_.p, half_.p, nsys);
        return;
    }
    pace_until_done(s, graph_, mirror, k, launched0, graph1_, horizon(-1));
}

void MassBatch::prepare(hipStream_t s, double* x_out) {
    if (nsys == 0) return;
    if (x_out != x_target_) {
        drop_graphs();
        x_target_ = x_out;
    }
    if (!graph_) capture(s);
}

void MassBatch::set_split(bool on) {
    on = on && nsys >= 2;
    if (on && !s2_) {
        DDPCA_HIP(hipStreamCreateWithFlags(&s2_, hipStreamNonBlocking));
        DDPCA_HIP(hipEventCreateWithFlags(&ev_fork_, hipEventDisableTiming));
        DDPCA_HIP(hipEventCreateWithFlags(&ev_join_, hipEventDisableTiming));
        sc_half_.alloc(2 * nsys);
        // a paired batch splits by pairs, so that a pair's shared matrix is read by one half
        const int nu = paired_ ? nsys / 2 : nsys;
        std::vector<int64_t> rows(nu, 0);
        std::vector<int> ord(nu);
        for (int i = 0; i < nsys; ++i) rows[i % nu] += cb_host_[i + 1] - cb_host_[i];
        for (int i = 0; i < nu; ++i) ord[i] = i;
        std::stable_sort(ord.begin(), ord.end(), [&](int a, int c) { return rows[a] > rows[c]; });
        half_host_.assign(nsys, 0);
        int64_t w[2] = {0, 0};
        for (int i : ord) {
            const int h = w[1] < w[0] ? 1 : 0;
            for (int j = i; j < nsys; j += nu) half_host_[j] = h;
            w[h] += rows[i];
        }
        half_.upload(half_host_);
    }
    if (on != split_) drop_graphs();
    split_ = on;
}

bool MassBatch::fuse_alpha() const {
    if (fuse_override >= 0) return fuse_override != 0;
    const char* ef = std::getenv("DDPCA_MCG_FUSE_ALPHA");
    if (ef && std::atoi(ef) == 0) return false;
    if (ef && std::atoi(ef) == 1) return true;
    for (int s = 0; s < nsys; ++s)
        if (cb_host_[s + 1] - cb_host_[s] > kMcgFuseMaxChunks) return false;
    return true;
}

void MassBatch::check() {
    last_iters = 0;
    expect_.resize(nsys);
    for (int i = 0; i < nsys; ++i) {
        if (mirror.host[i].fail) {
            solved_ = false;
            throw ApiError(DDPCA_ENUMERIC, "surface mass CG breakdown in system " + std::to_string(i));
        }
        expect_[i] = mirror.host[i].iter;  // paces the next solve's tail
        const int64_t ck = cheb_used_ ? (int64_t)cheb_ks_[i] : 0;
        last_iters = std::max<int64_t>(last_iters, mirror.host[i].iter + ck);
        if (solved_) {
            int64_t mit = mirror.host[i].iter;
            if (pair_used_) mit = i < nsys / 2 ? std::max(mit, mirror.host[i + nsys / 2].iter) : 0;
            alg_bytes += init_bytes_[i] + (double)mirror.host[i].iter * it_bytes_[i] + (double)mit * mat_bytes_[i];
            // Chebyshev: init (b, D^-1 read; x, r, d written) + per step (d gathered once, read;
            // x, r read + written; D^-1 read; d' written: 56 B per row) + the matrix once per
            // pair + the restart (b, r, D^-1 read; z, p, q written)
            if (cheb_used_)
                alg_bytes += init_bytes_[i] * (40.0 / 56.0) + (double)ck * (it_bytes_[i] * (56.0 / 112.0)) +
                             (pair_used_ ? (i < nsys / 2 ? (double)ck * mat_bytes_[i] : 0.0) : (double)ck * mat_bytes_[i]) +
                             init_bytes_[i] * (48.0 / 56.0);
        }
    }
    solved_ = false;
}

int64_t MassBatch::horizon(int half) const {
    const char* e = std::getenv("DDPCA_TAIL_PACING");
    if ((e && std::atoi(e) == 0) || (int)expect_.size() != nsys) return INT64_MAX;
    int64_t h = 0;
    for (int i = 0; i < nsys; ++i) {
        if (half >= 0 && half_host_[i] != half) continue;
        if (expect_[i] <= 0) return INT64_MAX;
        h = std::max(h, expect_[i]);
    }
    return h;
}

void MassBatch::drop_graphs() {
    for (hipGraphExec_t* g : {&graph_h_[0], &graph_h_[1], &graph1_h_[0], &graph1_h_[1], &graph1_, &cgraph_}) {
        if (*g) (void)hipGraphExecDestroy(*g);
        *g = nullptr;
    }
    if (graph_ && !split_) (void)hipGraphExecDestroy(graph_);  // (split: graph_ aliases graph_h_[0])
    graph_ = nullptr;
}

void MassBatch::plan_cheb(double rtol) {
    cheb_rtol_ = rtol;
    ChebPlan C = cheb_plan(lam_lo_, lam_hi_, rtol);
    cheb_ks_ = C.ks;
    cheb_k_ = C.K;
    // past kChebMax steps this tolerance runs the plain CG (capture() skips the Chebyshev
    // graph); cheb_ stays set, so a later solve at a looser tolerance plans it again
    if (C.K > kChebMax) return;
    ccoef_.upload(C.coef);
    cith_.upload(C.ith);
    ckmax_.upload(cheb_ks_);
}

void MassBatch::capture(hipStream_t s) {
    // DDPCA_MCG_PAIR=0: the unpaired kernels on a paired batch (bit-identical, A/B and tests)
    const char* ep = std::getenv("DDPCA_MCG_PAIR");
    const bool pair = pair_used_ = paired_ && !(ep && std::atoi(ep) == 0);
    if (cheb_ && cheb_k_ > 0 && cheb_k_ <= kChebMax) cgraph_ = capture_cheb(s, pair);
    if (split_) {
        for (int h = 0; h < 2; ++h) graph_h_[h] = capture_cg(s, pair, sc_half_.p + h * nsys, k);
        for (int h = 0; k > 1 && h < 2; ++h) graph1_h_[h] = capture_cg(s, pair, sc_half_.p + h * nsys, 1);
        graph_ = graph_h_[0];  // marks the capture done (destroyed through graph_h_)
        return;
    }
    graph_ = capture_cg(s, pair, sc.p, k);
    if (k > 1) graph1_ = capture_cg(s, pair, sc.p, 1);
}

hipGraphExec_t MassBatch::capture_cheb(hipStream_t s, bool pair) {
    EllArgs e{slots.p, off.p, col.p, val.p, csys.p, dinv.p, nch};
    return capture_graph(s, [&] {
        hipLaunchKernelGGL(k_mcheb_init, dim3(nb256(nrow)), dim3(256), 0, s, b.p, dinv.p, cith_.p, csys.p, x_target_, r.p,
                           z.p, nrow);
        double* d[2] = {z.p, p.p};
        for (int64_t kk = 0; kk < cheb_k_; ++kk)
            with_pairing(pair, nrow, nch, [&](auto P, int64_t R, int64_t n) {
                hipLaunchKernelGGL(k_mcheb_step<decltype(P)::value>, dim3(ceil_div(n, 4)), dim3(256), 0, s, e, ccoef_.p,
                                   ckmax_.p, nsys, (int)kk, (const double*)d[kk & 1], d[(kk + 1) & 1], x_target_, r.p, R, n);
            });
        hipLaunchKernelGGL(k_mcg_restart, dim3(nb256(nrow)), dim3(256), 0, s, b.p, dinv.p, r.p, z.p, p.p, q.p, partial.p,
                           partial.p + 2 * nch, nrow);
        hipLaunchKernelGGL(k_mcg_fin_restart, dim3(nsys), dim3(256), 0, s, partial.p, partial.p + 2 * nch, cb.p, sc.p,
                           mirror.dev);
    });
}

hipGraphExec_t MassBatch::capture_cg(hipStream_t s, bool pair, PcgScal* scp, int64_t iters) {
    EllArgs e{slots.p, off.p, col.p, val.p, csys.p, dinv.p, nch};
    const bool fa = fuse_alpha();
    double* ppq = partial.p + 2 * nch;  // p.q per chunk
    auto spmv = [&](double* part, int stride) {
        with_pairing(pair, nrow, nch, [&](auto P, int64_t R, int64_t n) {
            hipLaunchKernelGGL(k_mcg_spmv<decltype(P)::value>, dim3(ceil_div(n, 4)), dim3(256), 0, s, e, scp, z.p, q.p, p.p,
                               part, stride, R, n);
        });
    };
    return capture_graph(s, [&] {
        for (int64_t it = 0; it < iters; ++it) {
            if (fa) {
                spmv(ppq, 1);
                hipLaunchKernelGGL(k_mcg_axpy_fa, dim3(nb256(nrow)), dim3(256), 0, s, e, scp, x_target_, r.p, z.p, p.p,
                                   q.p, partial.p, (const double*)ppq, cb.p, mirror.dev);
            } else {
                spmv(partial.p, 2);
                hipLaunchKernelGGL(k_mcg_fin, dim3(nsys), dim3(256), 0, s, (int)kMcgAlpha, partial.p, cb.p, scp, mirror.dev);
                hipLaunchKernelGGL(k_mcg_axpy, dim3(nb256(nrow)), dim3(256), 0, s, e, scp, x_target_, r.p, z.p, p.p, q.p,
                                   partial.p);
            }
            hipLaunchKernelGGL(k_mcg_fin, dim3(nsys), dim3(256), 0, s, (int)kMcgBeta, partial.p, cb.p, scp, mirror.dev);
        }
    });
}

}  // namespace ddpca
