// MGPIS device path: the setup of a handle -- the plans of mgpis_plan.cpp uploaded level by level,
// the dense coarse inverses (device_dense.hip), the work buffers, the byte model's inputs
// (mgpis_bytes.hpp) and the smoother's spectral estimate.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>

#include "device_dense.hpp"
#include "device_mgpis.hpp"
#include "mgpis_device_fn.hpp"
#include "mgpis_launch.hpp"

namespace ddpca {

namespace {
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
}  // namespace

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
    // what the byte model (mgpis_bytes.cpp) reads of this handle, now that the copies are settled
    bytes_.lev.resize(nlev);
    for (int l = 0; l < nlev; ++l) {
        MgpisBytes::Level& B = bytes_.lev[l];
        static_cast<LevelShape&>(B) = lev[l];
        static_cast<TransferShape&>(B) = lev[l];
        B.vt = vc_type(l);
        B.col16 = lev[l].col16.p != nullptr;
        B.x4 = lev[l].x4a.p != nullptr;
    }
    static_cast<ColourShape&>(bytes_.gs) = gs;
    bytes_.gs.vt = vc_type(nlev - 1);
    bytes_.gs.col16 = gs.col16.p != nullptr;
    bytes_.gs.x4 = gs.x4.p != nullptr;
    bytes_.gs.r4 = gs.r4.p != nullptr;
    bytes_.nu = opt.nu;
    bytes_.smoother = opt.smoother;
    bytes_.clev = clev;
    bytes_.ainv32 = ainv32.p != nullptr;
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

}  // namespace ddpca
