// MGPIS device path: the PCG recurrence over the batch -- its vector and scalar kernels, the
// captured iteration graphs, the split of the batch over streams and the solve's host side.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <string>

#include "device_mgpis.hpp"
#include "mgpis_device_fn.hpp"
#include "mgpis_launch.hpp"

namespace ddpca {

namespace {

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
    double s = wsum((a[0] + a[1]) + (a[2] + a[3]));
    double s2 = wsum((b[0] + b[1]) + (b[2] + b[3]));
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
}  // namespace

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
