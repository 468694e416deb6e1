// Batched surface-mass solver of the ADMM loop (the reference's interface mass solves,
// MCONTACT.h:2671-2704): a Jacobi-PCG over every owned side's system at once, ELL-64 rows,
// per-system scalars in PcgScal.  Kernels and member definitions: device_mass.hip; host setup:
// mass_plan.hpp.
#pragma once
#include "device_mgpis.hpp"  // PcgScal
#include "mass_plan.hpp"

namespace ddpca {

// One graph of `k` CG iterations over every system, replayed until every system reports done
// through the host-mapped mirror.  Chebyshev mode (cheb_, the default where every system's steps
// fit kChebMax): a fixed-length Chebyshev iteration first, one launch per step, then the CG from
// its iterate -- usually converged at its first check.
class MassBatch {
public:
    int nsys = 0;
    int64_t nrow = 0, nch = 0;
    DevBuf<int32_t> slots, col, csys;
    DevBuf<int64_t> off, cb;
    DevBuf<double> val, dinv, b, x, r, z, p, q, partial;
    DevBuf<PcgScal> sc;
    PcgScal* sc_host = nullptr;
    MirrorBuf mirror;
    int64_t k = 8;
    int64_t last_iters = 0;
    double alg_bytes = 0.0;  // accumulated by check(): init + iterations of every system
    // Chebyshev mode: spectral bounds per system from build(), steps from the first solve's rtol
    bool cheb_ = false;
    int64_t cheb_k_ = 0;                       // steps of the captured Chebyshev graph (max over systems)
    std::vector<double> lam_lo_, lam_hi_;      // D^-1 M spectrum bounds used, per system
    std::vector<int32_t> cheb_ks_;             // steps per system

    ~MassBatch();

    // A[i] = system i (rows m_i), placed at rows roff[i] (multiples of 64) of nrow_total.
    void build(const std::vector<const Csr*>& A, const std::vector<int64_t>& roff, int64_t nrow_total);

    // x_out (nrow) = A^-1 b.  Asynchronous on `s` except for the host pacing of replays.
    void solve(hipStream_t s, double* x_out, double rtol, int64_t maxit);

    // capture the solve's graphs now (create time, one thread) for solves into x_out: the first
    // solve of an in-process rank then captures nothing while the other rank threads run
    void prepare(hipStream_t s, double* x_out);

    // Two-stream split of the systems (as MgpisDevice::set_split): two halves of equal rows, each
    // half's CG iterations a graph of its own on its own stream, on a copy of the scalars where
    // the other half's systems are done -- the latency-bound launches of the two halves overlap.
    void set_split(bool on);

    // alpha inside k_mcg_axpy_fa: default while every system has at most kMcgFuseMaxChunks chunks
    // (each wave re-reads its system's p.q partials); DDPCA_MCG_FUSE_ALPHA=0 forces the separate
    // k_mcg_fin launch, =1 the fused form at any size (read at graph capture)
    int fuse_override = -1;  // ddpca_mass_solve: 0 / 1 forces the form (tests), -1 the rule above
    bool fuse_alpha() const;

    // after the stream synchronised: iterations of the last solve, breakdown check
    void check();

private:
    hipGraphExec_t graph_ = nullptr;
    hipGraphExec_t graph_h_[2] = {nullptr, nullptr};
    // one-iteration graphs for the tail (MgpisDevice::graph1_): past the systems' previous
    // iteration counts the host queues single iterations two ahead of the slowest system
    hipGraphExec_t graph1_ = nullptr;
    hipGraphExec_t graph1_h_[2] = {nullptr, nullptr};
    std::vector<int64_t> expect_;
    int64_t horizon(int half) const;
    void drop_graphs();
    double* x_target_ = nullptr;
    hipGraphExec_t cgraph_ = nullptr;  // Chebyshev: init, steps, CG restart
    double cheb_rtol_ = -1.0;
    bool cheb_used_ = false;
    DevBuf<double> ccoef_, cith_;
    DevBuf<int32_t> ckmax_;
    void plan_cheb(double rtol);  // mass_plan.hpp cheb_plan for this tolerance, uploaded
    bool split_ = false;
    hipStream_t s2_ = nullptr;
    hipEvent_t ev_fork_ = nullptr, ev_join_ = nullptr;
    DevBuf<PcgScal> sc_half_;
    DevBuf<int32_t> half_;
    std::vector<int> half_host_;
    std::vector<int64_t> cb_host_;
    std::vector<double> init_bytes_, it_bytes_, mat_bytes_;
    bool solved_ = false;
    bool paired_ = false, pair_used_ = false;
    void capture(hipStream_t s);
    hipGraphExec_t capture_cheb(hipStream_t s, bool pair);
    hipGraphExec_t capture_cg(hipStream_t s, bool pair, PcgScal* scp, int64_t iters);
};

}  // namespace ddpca
