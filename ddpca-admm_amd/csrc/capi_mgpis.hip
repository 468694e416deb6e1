// C ABI: MGPIS device solver entry points (mgpis_gpu_*), see include/ddpca_amd.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ddpca_amd.h"
#include "device_mgpis.hpp"
#include "problem.hpp"
#include "subdomain_ops.hpp"

using namespace ddpca;

struct ddpca_mgpis {
    std::unique_ptr<MgpisDevice> dev;
};

namespace {

mgpis_options_t resolve(const mgpis_options_t* opt) {
    mgpis_options_t o;
    mgpis_default_options(&o);
    if (opt) o = *opt;
    return o;
}

// The reference calls CG_SOLV on different MGPIS objects from an omp parallel for
// (MCONTACT.h:2511-2531): every graph a solve replays is captured here, on the creating
// thread, so a solve only replays (no capture on a solving thread), and the
// solve's condensed staging buffer is allocated here too (no hipMalloc / hipFree per solve).
std::unique_ptr<MgpisDevice> finish_create(std::unique_ptr<MgpisDevice> d) {
    d->prepare_graphs(0);
    if (!d->no_coarse) d->prepare_graphs(1);
    int64_t n = 0;
    for (int64_t f : d->nfree) n += f;
    d->stage.alloc((size_t)std::max<int64_t>(n, 1));
    return d;
}

std::unique_ptr<MgpisDevice> single(int device, const std::vector<int64_t>& nn, const std::vector<const Bsr3*>& B,
                                    const std::vector<uint8_t>& fr, const std::vector<const Stencil*>& S,
                                    const mgpis_options_t* opt) {
    SubdomainOps ops;
    ops.nnodes = nn;
    ops.K = B;
    ops.dof_free = fr.data();
    ops.S = S;
    return finish_create(std::make_unique<MgpisDevice>(device, std::vector<SubdomainOps>{ops}, resolve(opt)));
}

// One MgpisDevice over the listed subdomains of an established problem, in the listed order
// (subdomain_ops: what the MCONTACT batch is built from); parts >= 2: set_split before the capture.
std::unique_ptr<MgpisDevice> from_problem(ddpca_problem_t p, int64_t ntv, const int64_t* tv, int device,
                                          const mgpis_options_t* opt, int parts) {
    if (!p || !tv || ntv < 1) throw ApiError(DDPCA_EINVAL, "null argument");
    Problem& P = *reinterpret_cast<Problem*>(p);
    if (!P.established) throw ApiError(DDPCA_ESTATE, "problem not established");
    if (parts != 0 && (parts < 2 || parts > kMaxParts)) throw ApiError(DDPCA_EINVAL, "parts must be 0 or 2 .. 4");
    std::vector<SubdomainOps> ops;
    for (int64_t i = 0; i < ntv; ++i) {
        if (tv[i] < 0 || tv[i] >= (int64_t)P.mc.multGrid.size()) throw ApiError(DDPCA_EINVAL, "subdomain index");
        if (!P.owned.empty() && !P.owned[tv[i]])
            throw ApiError(DDPCA_ESTATE, "subdomain " + std::to_string(tv[i]) + " was not established");
        ops.push_back(subdomain_ops(P.mc.multGrid[tv[i]]));
    }
    auto d = std::make_unique<MgpisDevice>(device, ops, resolve(opt));
    if (parts >= 2) d->set_split(true, parts);
    return finish_create(std::move(d));
}

// first condensed entry of every member in the batch vectors (nsub + 1)
std::vector<int64_t> member_offsets(const MgpisDevice& D) {
    std::vector<int64_t> off(D.nsub + 1, 0);
    for (int s = 0; s < D.nsub; ++s) off[s + 1] = off[s] + D.nfree[s];
    return off;
}

// condensed host vector (member after member) -> the fine level's batch nodal layout, through stage
void upload_members(MgpisDevice& D, const std::vector<int64_t>& off, const double* host, double* full) {
    DDPCA_HIP(hipMemcpyAsync(D.stage.p, host, off[D.nsub] * sizeof(double), hipMemcpyHostToDevice, D.stream));
    for (int s = 0; s < D.nsub; ++s) D.scatter_free(s, D.stage.p + off[s], full);
}

void download_members(MgpisDevice& D, const std::vector<int64_t>& off, const double* full, double* host) {
    for (int s = 0; s < D.nsub; ++s) D.gather_free(s, full, D.stage.p + off[s]);
    DDPCA_HIP(hipMemcpyAsync(host, D.stage.p, off[D.nsub] * sizeof(double), hipMemcpyDeviceToHost, D.stream));
    DDPCA_HIP(hipStreamSynchronize(D.stream));
}

}  // namespace

extern "C" {

void mgpis_default_options(mgpis_options_t* opt) {
    opt->smoother = 1;
    opt->nu = 1;
    opt->omega = -1.7;  // 1.7 / lambda_max: damping sweep, profiles/r01_sweep_omega.txt
    opt->coarse_level = -1;
    opt->iters_per_graph = 4;
    opt->warm_start = 0;
    opt->precond_fp32 = 0;
    opt->table_mode = 1;
}

int ddpca_gpu_available(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return 0;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) return 0;
    return std::strncmp(prop.gcnArchName, "gfx950", 6) == 0 ? 1 : 0;
}

int mgpis_gpu_create(int device, int nlev, const int64_t* nnodes, const int64_t* nfree,
                     const int32_t* const* free_dof, const int64_t* const* K_ptr, const int32_t* const* K_col,
                     const double* const* K_val, const int64_t* const* S_ptr, const int32_t* const* S_col,
                     const double* const* S_w, const mgpis_options_t* opt, mgpis_t* out) {
    return guarded([&] {
        if (nlev < 1 || !nnodes || !nfree || !free_dof || !K_ptr || !K_col || !K_val || !out)
            throw ApiError(DDPCA_EINVAL, "null argument");
        std::vector<Bsr3> B(nlev);
        std::vector<Stencil> S(nlev - 1);
        for (int l = 0; l < nlev; ++l) B[l] = condensed_to_bsr3(nnodes[l], nfree[l], free_dof[l], K_ptr[l], K_col[l], K_val[l]);
        for (int l = 0; l + 1 < nlev; ++l) S[l] = make_stencil(nnodes[l + 1], nnodes[l], S_ptr[l], S_col[l], S_w[l]);
        const int64_t nn = nnodes[nlev - 1];
        std::vector<uint8_t> fr(3 * nn, 0);
        for (int64_t r = 0; r < nfree[nlev - 1]; ++r) fr[free_dof[nlev - 1][r]] = 1;
        std::vector<int64_t> nn_v(nnodes, nnodes + nlev);
        std::vector<const Bsr3*> Bp;
        std::vector<const Stencil*> Sp;
        for (auto& b : B) Bp.push_back(&b);
        for (auto& s : S) Sp.push_back(&s);
        auto h = std::make_unique<ddpca_mgpis>();
        h->dev = single(device, nn_v, Bp, fr, Sp, opt);
        *out = h.release();
    });
}

int mgpis_gpu_create_prol(int device, int nlev, const int64_t* nnodes, const int64_t* nfree,
                          const int32_t* const* free_dof, const int64_t* const* K_ptr, const int32_t* const* K_col,
                          const double* const* K_val, const int64_t* const* P_ptr, const int32_t* const* P_col,
                          const double* const* P_val, const mgpis_options_t* opt, mgpis_t* out) {
    return guarded([&] {
        if (nlev < 1 || !nnodes || !nfree || !free_dof || !K_ptr || !K_col || !K_val || !out)
            throw ApiError(DDPCA_EINVAL, "null argument");
        if (nlev > 1 && (!P_ptr || !P_col || !P_val)) throw ApiError(DDPCA_EINVAL, "null realProl");
        std::vector<Bsr3> B(nlev);
        std::vector<Stencil> S(nlev - 1);
        for (int l = 0; l < nlev; ++l) B[l] = condensed_to_bsr3(nnodes[l], nfree[l], free_dof[l], K_ptr[l], K_col[l], K_val[l]);
        for (int l = 0; l + 1 < nlev; ++l) {
            try {
                S[l] = prol_to_stencil(nnodes[l + 1], nnodes[l], nfree[l + 1], free_dof[l + 1], free_dof[l], P_ptr[l],
                                       P_col[l], P_val[l]);
            } catch (const std::invalid_argument& e) {
                throw ApiError(DDPCA_EINVAL, e.what());
            }
        }
        const int64_t nn = nnodes[nlev - 1];
        std::vector<uint8_t> fr(3 * nn, 0);
        for (int64_t r = 0; r < nfree[nlev - 1]; ++r) fr[free_dof[nlev - 1][r]] = 1;
        std::vector<int64_t> nn_v(nnodes, nnodes + nlev);
        std::vector<const Bsr3*> Bp;
        std::vector<const Stencil*> Sp;
        for (auto& b : B) Bp.push_back(&b);
        for (auto& s : S) Sp.push_back(&s);
        auto h = std::make_unique<ddpca_mgpis>();
        h->dev = single(device, nn_v, Bp, fr, Sp, opt);
        *out = h.release();
    });
}

int mgpis_gpu_create_bsr3(int device, int nlev, const int64_t* nnodes, const int64_t* const* B_ptr,
                          const int32_t* const* B_col, const double* const* B_val, const uint8_t* dof_free,
                          const int64_t* const* S_ptr, const int32_t* const* S_col, const double* const* S_w,
                          const mgpis_options_t* opt, mgpis_t* out) {
    return guarded([&] {
        if (nlev < 1 || !nnodes || !B_ptr || !B_col || !B_val || !dof_free || !out) throw ApiError(DDPCA_EINVAL, "null argument");
        std::vector<Bsr3> B(nlev);
        std::vector<Stencil> S(nlev - 1);
        for (int l = 0; l < nlev; ++l) {
            B[l].nb = B[l].mb = nnodes[l];
            B[l].ptr.assign(B_ptr[l], B_ptr[l] + nnodes[l] + 1);
            B[l].col.assign(B_col[l], B_col[l] + B_ptr[l][nnodes[l]]);
            B[l].val.assign(B_val[l], B_val[l] + 9 * B_ptr[l][nnodes[l]]);
        }
        for (int l = 0; l + 1 < nlev; ++l) S[l] = make_stencil(nnodes[l + 1], nnodes[l], S_ptr[l], S_col[l], S_w[l]);
        std::vector<uint8_t> fr(dof_free, dof_free + 3 * nnodes[nlev - 1]);
        std::vector<int64_t> nn_v(nnodes, nnodes + nlev);
        std::vector<const Bsr3*> Bp;
        std::vector<const Stencil*> Sp;
        for (auto& b : B) Bp.push_back(&b);
        for (auto& s : S) Sp.push_back(&s);
        auto h = std::make_unique<ddpca_mgpis>();
        h->dev = single(device, nn_v, Bp, fr, Sp, opt);
        *out = h.release();
    });
}

int ddpca_problem_mgpis(ddpca_problem_t p, int64_t tv, int device, const mgpis_options_t* opt, mgpis_t* out) {
    return ddpca_problem_mgpis_batch(p, 1, &tv, device, opt, 0, out);
}

int ddpca_problem_mgpis_batch(ddpca_problem_t p, int64_t ntv, const int64_t* tv, int device, const mgpis_options_t* opt,
                              int parts, mgpis_t* out) {
    return guarded([&] {
        if (!out) throw ApiError(DDPCA_EINVAL, "null argument");
        auto h = std::make_unique<ddpca_mgpis>();
        h->dev = from_problem(p, ntv, tv, device, opt, parts);
        *out = h.release();
    });
}

int mgpis_gpu_solve(mgpis_t h, const double* b, double* x, int prec, double rtol, int64_t maxit, int64_t* iters,
                    double* relres) {
    int64_t it = 0;
    int rc = guarded([&] {
        if (!h || !b || !x) throw ApiError(DDPCA_EINVAL, "null argument");
        if (prec != 0 && prec != 1) throw ApiError(DDPCA_EINVAL, "prec must be 0 or 1");
        MgpisDevice& D = *h->dev;
        select_device(D.device);
        if (prec == 1 && D.no_coarse) throw ApiError(DDPCA_ESTATE, "one-level handle without a coarse inverse: diagonal preconditioner only");
        // stream-ordered only: the handle's own staging buffer and stream, graphs captured at create
        DDPCA_HIP(hipMemcpyAsync(D.stage.p, b, D.nfree[0] * sizeof(double), hipMemcpyHostToDevice, D.stream));
        D.scatter_free(0, D.stage.p, D.bs.p);
        D.pcg_solve(prec, rtol, {maxit});
        it = D.sc_host[0].iter;
        D.gather_free(0, D.xs.p, D.stage.p);
        DDPCA_HIP(hipMemcpyAsync(x, D.stage.p, D.nfree[0] * sizeof(double), hipMemcpyDeviceToHost, D.stream));
        DDPCA_HIP(hipStreamSynchronize(D.stream));
        if (iters) *iters = it;
        if (relres) *relres = D.sc_host[0].bb > 0 ? std::sqrt(D.sc_host[0].rr / D.sc_host[0].bb) : 0.0;
    });
    if (rc != 0) return rc;
    return (maxit > 0 && it >= maxit) ? (int)std::min<int64_t>(it, 1 << 30) : 0;
}

}  // extern "C"
namespace {
// Shared shell of the non-CG drivers: condensed host b -> device nodal layout, run, gather x.
template <typename F>
int run_driver(mgpis_t h, const double* b, double* x, int64_t maxit, int64_t* iters, F body) {
    int64_t it = 0;
    int rc = guarded([&] {
        if (!h || !b || !x) throw ApiError(DDPCA_EINVAL, "null argument");
        if (maxit < 0) throw ApiError(DDPCA_EINVAL, "maxit must be >= 0");
        MgpisDevice& D = *h->dev;
        if (D.nsub != 1) throw ApiError(DDPCA_EINVAL, "driver needs a one-subdomain handle");
        select_device(D.device);
        DevBuf<double> tmp;
        tmp.upload(b, D.nfree[0]);
        D.bs.zero(D.stream);
        D.scatter_free(0, tmp.p, D.bs.p);
        it = body(D, D.bs.p, D.xs.p);
        D.gather_free(0, D.xs.p, tmp.p);
        DDPCA_HIP(hipMemcpyAsync(x, tmp.p, D.nfree[0] * sizeof(double), hipMemcpyDeviceToHost, D.stream));
        DDPCA_HIP(hipStreamSynchronize(D.stream));
        if (iters) *iters = it;
    });
    if (rc != 0) return rc;
    return (maxit > 0 && it >= maxit) ? (int)std::min<int64_t>(it, 1 << 30) : 0;
}
}  // namespace
extern "C" {

int mgpis_gpu_mult_solve(mgpis_t h, const double* b, double* x, int64_t maxit, int64_t* iters, double* relres) {
    return run_driver(h, b, x, maxit, iters, [&](MgpisDevice& D, const double* bd, double* xd) {
        return krylov_mult_solv(D, bd, xd, maxit, relres);
    });
}

int mgpis_gpu_bicgstab(mgpis_t h, const double* b, double* x, int prec, double rtol, int64_t maxit, int64_t* iters,
                       double* relres, int* breakdown) {
    if (prec != 0 && prec != 1) return guarded([] { throw ApiError(DDPCA_EINVAL, "prec must be 0 or 1"); });
    return run_driver(h, b, x, maxit, iters, [&](MgpisDevice& D, const double* bd, double* xd) {
        return krylov_bicgstab(D, prec, bd, xd, rtol, maxit, relres, breakdown);
    });
}

int mgpis_gpu_gmres(mgpis_t h, const double* b, double* x, int prec, double rtol, int64_t maxit, int64_t restart,
                    int64_t* iters, double* relres) {
    if (prec != 0 && prec != 1) return guarded([] { throw ApiError(DDPCA_EINVAL, "prec must be 0 or 1"); });
    return run_driver(h, b, x, maxit, iters, [&](MgpisDevice& D, const double* bd, double* xd) {
        return krylov_gmres(D, prec, bd, xd, rtol, maxit, restart, relres);
    });
}

int mgpis_gpu_spmv(mgpis_t h, int level, const double* x, double* y) { return mgpis_gpu_spmv_copy(h, level, 0, x, y); }

int mgpis_gpu_spmv_copy(mgpis_t h, int level, int vcycle_copy, const double* x, double* y) {
    return guarded([&] {
        if (!h || !x || !y) throw ApiError(DDPCA_EINVAL, "null argument");
        MgpisDevice& D = *h->dev;
        select_device(D.device);
        if (level < 0 || level >= (int)D.lev.size()) throw ApiError(DDPCA_EINVAL, "level");
        if (level != (int)D.lev.size() - 1) throw ApiError(DDPCA_EINVAL, "condensed spmv is defined on the fine level");
        if (vcycle_copy && D.vc_type(level) == kVal64) throw ApiError(DDPCA_EINVAL, "no reduced-precision V-cycle copy (precond_fp32 = 0)");
        DevBuf<double> tmp, full_x, full_y;
        tmp.upload(x, D.nfree[0]);
        full_x.alloc(3 * D.lev.back().nn);
        full_y.alloc(3 * D.lev.back().nn);
        D.scatter_free(0, tmp.p, full_x.p);
        D.spmv(level, full_x.p, full_y.p, vcycle_copy != 0);
        D.gather_free(0, full_y.p, tmp.p);
        DDPCA_HIP(hipMemcpyAsync(y, tmp.p, D.nfree[0] * sizeof(double), hipMemcpyDeviceToHost, D.stream));
        DDPCA_HIP(hipStreamSynchronize(D.stream));
    });
}

int mgpis_gpu_vcycle(mgpis_t h, const double* r, double* z) {
    return guarded([&] {
        if (!h || !r || !z) throw ApiError(DDPCA_EINVAL, "null argument");
        MgpisDevice& D = *h->dev;
        select_device(D.device);
        DDPCA_HIP(hipMemcpyAsync(D.stage.p, r, D.nfree[0] * sizeof(double), hipMemcpyHostToDevice, D.stream));
        D.scatter_free(0, D.stage.p, D.rs.p);
        DDPCA_HIP(hipMemsetAsync(D.sc.p, 0, sizeof(PcgScal), D.stream));  // done = 0
        D.vcycle(D.rs.p, D.zs.p, false);
        D.gather_free(0, D.zs.p, D.stage.p);
        DDPCA_HIP(hipMemcpyAsync(z, D.stage.p, D.nfree[0] * sizeof(double), hipMemcpyDeviceToHost, D.stream));
        DDPCA_HIP(hipStreamSynchronize(D.stream));
    });
}

int mgpis_gpu_batch_vcycle(mgpis_t h, const double* r, double* z, const int32_t* done) {
    return guarded([&] {
        if (!h || !r || !z) throw ApiError(DDPCA_EINVAL, "null argument");
        MgpisDevice& D = *h->dev;
        select_device(D.device);
        if (D.no_coarse) throw ApiError(DDPCA_ESTATE, "one-level handle without a coarse inverse: no V-cycle");
        const std::vector<int64_t> off = member_offsets(D);
        upload_members(D, off, r, D.rs.p);
        upload_members(D, off, z, D.zs.p);
        std::vector<PcgScal> sc(D.nsub, PcgScal{});
        for (int s = 0; s < D.nsub; ++s) sc[s].done = done && done[s] ? 1 : 0;
        DDPCA_HIP(hipMemcpyAsync(D.sc.p, sc.data(), D.nsub * sizeof(PcgScal), hipMemcpyHostToDevice, D.stream));
        D.vcycle(D.rs.p, D.zs.p, false);
        download_members(D, off, D.zs.p, z);
    });
}

int mgpis_gpu_batch_solve(mgpis_t h, const double* b, double* x, int prec, double rtol, const int64_t* maxit, int warm,
                          int64_t* iters, double* relres, int32_t* fail) {
    return guarded([&] {
        if (!h || !b || !x || !maxit) throw ApiError(DDPCA_EINVAL, "null argument");
        if (prec != 0 && prec != 1) throw ApiError(DDPCA_EINVAL, "prec must be 0 or 1");
        MgpisDevice& D = *h->dev;
        select_device(D.device);
        if (prec == 1 && D.no_coarse) throw ApiError(DDPCA_ESTATE, "one-level handle without a coarse inverse: diagonal preconditioner only");
        const std::vector<int64_t> off = member_offsets(D);
        upload_members(D, off, b, D.bs.p);
        if (warm) upload_members(D, off, x, D.xs.p);
        D.pcg_begin(prec, rtol, std::vector<int64_t>(maxit, maxit + D.nsub), warm != 0);
        D.pcg_wait(prec, 0);
        D.pcg_fetch();
        DDPCA_HIP(hipStreamSynchronize(D.stream));
        for (int s = 0; s < D.nsub; ++s) {
            const PcgScal& c = D.sc_host[s];
            if (iters) iters[s] = c.iter;
            if (relres) relres[s] = c.bb > 0 ? std::sqrt(c.rr / c.bb) : 0.0;
            if (fail) fail[s] = c.fail;
        }
        download_members(D, off, D.xs.p, x);
        D.pcg_check();  // a breakdown throws DDPCA_ENUMERIC here, the outputs above already filled
    });
}

int mgpis_gpu_info(mgpis_t h, int64_t* out7) {
    return guarded([&] {
        MgpisDevice& D = *h->dev;
        out7[0] = (int64_t)D.lev.size();
        const double lmax = D.lev.size() > 1 ? D.lev.back().lmax[0] : 0.0;
        out7[1] = D.nfree[0];
        out7[2] = D.lev.back().nnzb;
        out7[3] = D.lev.back().nch;
        const double scale = D.opt.omega < 0.0 ? -D.opt.omega : 4.0 / 3.0;
        out7[4] = (int64_t)((D.opt.omega > 0.0 ? D.opt.omega : lmax > 0.0 ? scale / lmax : 1.0) * 1e6);
        out7[5] = (int64_t)(lmax * 1e6);
        out7[6] = D.device;
    });
}

int64_t mgpis_gpu_vcycle_info(mgpis_t h, const char* what, int level, void* out, int64_t cap) {
    int64_t count = 0;
    const int rc = guarded([&] {
        if (!h || !what) throw ApiError(DDPCA_EINVAL, "null argument");
        MgpisDevice& D = *h->dev;
        select_device(D.device);
        const int nlev = (int)D.lev.size();
        const std::string w(what);
        // copy v out (out == NULL: the size query)
        auto put = [&](const auto& v) {
            count = (int64_t)v.size();
            if (!out) return;
            if (cap < count) throw ApiError(DDPCA_EINVAL, "vcycle_info: out is too small");
            if (count) std::memcpy(out, v.data(), v.size() * sizeof(v[0]));
        };
        if (w == "lmax" || w == "coef") {
            // (level 0 is never smoothed: no spectrum estimate, no coefficient table)
            if (level < 1 || level >= nlev) throw ApiError(DDPCA_EINVAL, "vcycle_info: level");
            if (w == "lmax") put(D.lev[level].lmax);
            else put(D.lev[level].coef.download());
        } else if (w == "colour") {
            // the colour of a node = the group of the colour chunk that sweeps it (GsFine::list,
            // rowidx: what the sweeps run over), mapped back through the device numbering
            const LevelDev& F = D.lev.back();
            std::vector<int32_t> dev(F.nn, -1);
            if (D.gs_fine()) {
                const std::vector<int32_t> list = D.gs.list.download(), rowidx = D.gs.rowidx.download();
                for (int k = 0; k < D.gs.ncol; ++k)
                    for (int64_t q = D.gs.first[k]; q < D.gs.first[k] + D.gs.count[k]; ++q)
                        for (int64_t lane = 0; lane < kChunk; ++lane) {
                            const int32_t rr = rowidx[(int64_t)list[q] * kChunk + lane];
                            if (rr >= 0) dev[rr] = k;
                        }
            }
            std::vector<int32_t> ref;
            for (int s = 0; s < D.nsub; ++s)
                for (int64_t i = 0; i < F.nloc[s]; ++i) ref.push_back(dev[F.noff[s] + D.fine_perm[s][i]]);
            put(ref);
        } else if (w == "levels") {
            std::vector<int32_t> v;
            for (int l = 0; l < nlev; ++l) {
                const LevelDev& L = D.lev[l];
                const bool x4 = (l == nlev - 1 && D.gs_fine()) ? D.gs.x4.p != nullptr : L.x4a.p != nullptr;
                for (int e : {D.clev, (int)L.lat, (int)(L.nrot != 0), (int)x4, D.vc_type(l)}) v.push_back(e);
            }
            put(v);
        } else if (w == "part") {
            std::vector<int32_t> v;
            for (int s = 0; s < D.nsub; ++s) v.push_back(D.part_of(s));
            put(v);
        } else if (w == "nfree") {
            put(D.nfree);
        } else {
            throw ApiError(DDPCA_EINVAL, "vcycle_info: unknown item");
        }
    });
    return rc != 0 ? rc : count;
}

int mgpis_gpu_bench_spmv(mgpis_t h, int variant, int reps, double* ms, double* bytes) {
    return guarded([&] {
        if (!h || !ms) throw ApiError(DDPCA_EINVAL, "null argument");
        MgpisDevice& D = *h->dev;
        select_device(D.device);
        *ms = D.bench_spmv(variant, reps);
        // 76 B per block + x gathered once (24 B/node) + per-node vector traffic of the mode:
        // y = Kx writes y; PCG reads/writes p, q; residual reads b, writes r; Chebyshev reads b,
        // x, d, the 9-entry block inverse and writes d, x_new
        const double per_node[4] = {24.0, 96.0, 48.0, 24.0 * 5.0 + 72.0};
        const int mode = (variant >> 2) & 3;
        const bool f32 = (variant & 16) != 0;
        if (bytes) *bytes = D.fine_matrix_bytes(0, !f32 ? kVal64 : D.vc_type((int)D.lev.size() - 1), false) + (24.0 + per_node[mode]) * (double)D.lev.back().nloc[0];
    });
}

int mgpis_gpu_destroy(mgpis_t h) {
    return guarded([&] { delete h; });
}

}  // extern "C"
