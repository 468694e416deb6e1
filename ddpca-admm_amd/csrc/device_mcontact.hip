// MCONTACT device path: the ADMM loop of CONTACT_ANALYSIS (MCONTACT.h:2493-2723) for the
// subdomains and interface sides owned by one rank (one process per GPU).
//
// Per iteration (same data flow as the reference):
//   body balance   b_tv = consForc + consOper (systTran_pena aux - systTran lambda)   (2514-2524)
//                  u_tv = OUTP_SUB1(MGPIS PCG(b_tv))                                 (2531-2533)
//                  -- every owned subdomain in ONE batched PCG (device_mgpis.hpp)
//   interface      gamma = 1/2 (L0 l0 - L1 l1 + R0 u0 - R1 u1 - pema g)              (2632-2636)
//                  -- each side contributes its half; sides on different ranks swap their
//                     halves with one RCCL send/recv pair over xGMI (no global collective)
//                  normal / Coulomb projection                                        (2637-2668)
//                  aux = (M^rho)^-1 (T^T u + M l + I gamma)                           (2671-2684)
//   Lagrange       l += M^-1 (T^T u - M^rho aux)                                      (2689-2704)
//   MONITOR        squared norms reduced on device, one small RCCL all-reduce,
//                  reference stopping logic on the host                               (2725-2845)
//
// Layout: one device workspace W = [u | aux, lambda | gamma] per rank.  u: displacements of all
// owned subdomains in the batch's fine layout (reference node order inside each subdomain);
// aux / lambda: all owned sides, each padded to 64 rows; gamma: every interface.  The three
// interface products (gamma, the aux right-hand side, the lambda right-hand side) of ALL owned
// sides are each ONE SELL-64 operator whose columns index W, so each is one coalesced launch.
// The surface mass solves (LDLT in the reference, < 120000 rows) run as ONE batched Jacobi-PCG
// over every owned side (ELL-64 rows, per-side scalars) to a 1e-14 relative residual
// (device_mass.hpp); the ranks' exchanges go through a Transport (device_transport.hpp).
// Everything runs on the batch's single stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <thread>

#include "../../include/ddpca_amd.h"
#include "admm_plan.hpp"
#include "device_dense.hpp"
#include "device_eigs.hpp"
#include "device_mass.hpp"
#include "device_mgpis.hpp"
#include "device_stress.hpp"
#include "device_transport.hpp"
#include "problem.hpp"
#include "subdomain_ops.hpp"

using namespace ddpca;

namespace {

// ------------------------------------------------------------------------------- kernels
__device__ __forceinline__ double csr_row(const int64_t* ptr, const int32_t* col, const double* val, const double* x,
                                          int64_t r) {
    double s = 0.0;
    for (int64_t k = ptr[r]; k < ptr[r + 1]; ++k) s += val[k] * x[col[k]];
    return s;
}

// y = x, 16 B per lane (n even: batch vectors are 3 * multiple-of-64 long, or 2R)
__global__ void k_copy2(double2* y, const double2* x, int64_t n2) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n2) y[i] = x[i];
}

// b[rows[i]] += sum_k val[k] W[col[k]]  (coupling of the body-balance RHS, surface rows only,
// ~50 entries each): 16 lanes per row, so a row's entries are read as one coalesced segment
__global__ __launch_bounds__(256) void k_cpl(const int32_t* rows, const int64_t* ptr, const int32_t* col,
                                             const double* val, const double* W, double* b, int64_t n) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int sl = threadIdx.x & 15;
    double s = 0.0;
    if (i < n)
        for (int64_t k = ptr[i] + sl; k < ptr[i + 1]; k += 16) s += val[k] * W[col[k]];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 16);
    if (i < n && sl == 0) b[rows[i]] += s;
}

// u = mask ? x : prescribed  (OUTP_SUB1 without rotations); x and mask in the solver's device
// node order, u and presc in the reference order (onode: device node -> reference node)
__global__ void k_outp(const double* x, const uint8_t* mask, const int32_t* onode, const double* presc, double* u,
                       int64_t nn) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nn) return;
    const uint8_t m = mask[i];
    const int64_t o = onode[i];
    for (int a = 0; a < 3; ++a) u[3 * o + a] = ((m >> a) & 1) ? x[3 * i + a] : presc[3 * o + a];
}

// y = a - b
__global__ void k_sub(const double* a, const double* b, double* y, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = a[i] - b[i];
}

__global__ void k_add(double* y, const double* x, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] += x[i];
}

// y[row] = sum_k val * W[col] (+ add[row]): one wavefront per 64 rows, slot-major (SELL-64)
__global__ __launch_bounds__(256) void k_sell_w(const int32_t* slots, const int64_t* off, const int32_t* col,
                                                const double* val, int64_t nch, const double* W, double* y,
                                                const double* add) {
    const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= nch) return;
    const int lane = threadIdx.x & 63;
    const int ns = slots[c];
    const int32_t* cp = col + off[c] * 64 + lane;
    const double* vp = val + off[c] * 64 + lane;
    double s = 0.0;
#pragma unroll 4
    for (int k = 0; k < ns; ++k)
        s += __builtin_nontemporal_load(vp + (int64_t)k * 64) * W[__builtin_nontemporal_load(cp + (int64_t)k * 64)];
    const int64_t row = c * 64 + lane;
    y[row] = add ? s + add[row] : s;
}

// normal / Coulomb projection at integration points (MCONTACT.h:2637-2668)
__global__ void k_project(double* g, int32_t* stat, int64_t nip, int comp, double fric) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nip) return;
    if (comp == 1) {
        g[q] = fmax(0.0, g[q]);
        stat[q] = 0;
        return;
    }
    double* v = g + 3 * q;
    if (fric < 0.0) {
        stat[q] = 0;
        return;
    }
    v[0] = fmax(0.0, v[0]);
    if (fric == 0.0) {
        stat[q] = 0;
        return;
    }
    if (v[0] > 0.0) {
        const double slid = fric * v[0];
        const double nt = sqrt(v[1] * v[1] + v[2] * v[2]);
        if (nt >= slid) {
            v[1] = slid / nt * v[1];
            v[2] = slid / nt * v[2];
            stat[q] = 1;
        } else {
            stat[q] = 2;
        }
    } else {
        v[1] = 0.0;
        v[2] = 0.0;
        stat[q] = 0;
    }
}

// ---- factored per-ip interface operators (host-built interfaces, Interface::factored).  Every
// row of inpoLagr, pemaInpo_r and inteInpo is an outer product of ONE integration point's shape
// values, basis and weight (mcontact.cpp BUILD, MCONTACT.h:570-714), so the gamma product and the
// inteInpo product are applied from the ip data -- 4 shape values, 4 + 4 node indices per side and
// the 3x3 basis per ip -- instead of streaming the 24 (frictional: 24 per row, 3 rows) stored
// entries of every gamma row.  Per-ip arrays are slot-major (x[slot * nip + q]).
struct IpSide {
    const double* M;     // 4 x nip shape values
    const int32_t* lam;  // 4 x nip: workspace index of the contact node's first lambda component
    const int32_t* u;    // 4 x nip: workspace index of the body node's first dof
};

// gamma[C q + m] = gcst + sum over owned sides s of h_s (inpoLagr_s lambda_s + pemaInpo_r_s u_s),
// h_0 = 1/2, h_1 = -1/2 (MCONTACT.h:2632-2636); one thread per ip
__global__ __launch_bounds__(256) void k_gamma_ip(const double* B, IpSide s0, IpSide s1, int own0, int own1, double p0,
                                                  double p1, double p2, int C, int64_t nip, const double* W,
                                                  double* gamma, const double* gcst) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nip) return;
    double b[3][3];
#pragma unroll
    for (int j = 0; j < 9; ++j) b[j / 3][j % 3] = B[(int64_t)j * nip + q];
    const double pen[3] = {p0, p1, p2};
    // gamma = (constant + side 0's half) + side 1's half, in that order whichever rank holds which
    // side (a cross-rank interface adds the received half to its own: the same two sums, and a + b
    // is b + a): the same bits on every rank layout
    double g[3] = {0.0, 0.0, 0.0};
    for (int m = 0; m < C; ++m) g[m] = gcst[C * q + m];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        if (!(s ? own1 : own0)) continue;
        const IpSide& S = s ? s1 : s0;
        const double h = s ? -0.5 : 0.5;
        double l[3] = {0.0, 0.0, 0.0}, u[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const double m = S.M[(int64_t)a * nip + q];
            const double* lp = W + S.lam[(int64_t)a * nip + q];
            const double* up = W + S.u[(int64_t)a * nip + q];
            l[0] += m * lp[0];
            if (C == 3) {
                l[1] += m * lp[1];
                l[2] += m * lp[2];
            }
            u[0] += m * up[0];
            u[1] += m * up[1];
            u[2] += m * up[2];
        }
        if (C == 1) {
            g[0] += h * (l[0] + pen[0] * (b[0][0] * u[0] + b[0][1] * u[1] + b[0][2] * u[2]));
        } else {
#pragma unroll
            for (int m = 0; m < 3; ++m)
                g[m] += h * ((b[m][0] * l[0] + b[m][1] * l[1] + b[m][2] * l[2]) +
                             pen[m] * (b[m][0] * u[0] + b[m][1] * u[1] + b[m][2] * u[2]));
        }
    }
    for (int m = 0; m < C; ++m) gamma[C * q + m] = g[m];
}

// y[dst[i]] += x[i]: the side-1 halves of rank-local interfaces onto their side-0 halves
__global__ void k_add_idx(double* y, const double* x, const int32_t* dst, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[dst[i]] += x[i];
}

// the projected traction in global components, T[3 q + k] = sum_m basis[m][k] gamma[3 q + m]
// (C = 1: T[q] = gamma[q]) -- what inteInpo's rows contract gamma with
__global__ void k_traction_ip(const double* B, const double* gamma, double* T, int C, int64_t nip) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nip) return;
    if (C == 1) {
        T[q] = gamma[q];
        return;
    }
    const double g0 = gamma[3 * q], g1 = gamma[3 * q + 1], g2 = gamma[3 * q + 2];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        T[3 * q + k] = B[(int64_t)k * nip + q] * g0 + B[(int64_t)(3 + k) * nip + q] * g1 + B[(int64_t)(6 + k) * nip + q] * g2;
}

// out[C a + k] = sum over the ips q touching contact node a of coef (= sgn w_q M_a(q)) T[C q + k]:
// inteInpo gamma (MCONTACT.h:2671-2684) node-major; a contact node collects up to ~1000 ips on
// refined contact faces, so one wavefront per node splits its list over the lanes
__global__ __launch_bounds__(256) void k_inpo_node(const int64_t* ptr, const int32_t* iq, const double* coef,
                                                   const double* T, int C, int64_t nnc, double* out) {
    const int64_t a = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (a >= nnc) return;
    const int lane = threadIdx.x & 63;
    double v0 = 0.0, v1 = 0.0, v2 = 0.0;
    for (int64_t e = ptr[a] + lane; e < ptr[a + 1]; e += 64) {
        const double c = coef[e];
        const double* t = T + (int64_t)C * iq[e];
        v0 += c * t[0];
        if (C == 3) {
            v1 += c * t[1];
            v2 += c * t[2];
        }
    }
    v0 = wsum(v0);
    if (C == 3) {
        v1 = wsum(v1);
        v2 = wsum(v2);
    }
    if (lane == 0) {
        out[C * a] = v0;
        if (C == 3) {
            out[C * a + 1] = v1;
            out[C * a + 2] = v2;
        }
    }
}

// All MONITOR pair norms of an iteration in two launches (instead of two per vector pair, 3.63 ->
// 3.40 ms interface step at the headline, profiles/r03ab): block b of k_pair_norms_all is block
// b - blk0[g] of segment g = bseg[b] (256 elements, the pair's squared difference and square), and
// k_reduce_pairs_all reduces segment g's blocks in one workgroup, a fixed order
struct NormSeg {
    const double* a;
    const double* o;
    int64_t n;
    int64_t blk0;  // first block of the segment in the batched grid
    int64_t nb;    // its blocks
    int64_t slot;  // moni slot (2 doubles)
};

__global__ void k_pair_norms_all(const NormSeg* seg, const int32_t* bseg, double* partial) {
    __shared__ double r1[4], r2[4];
    const NormSeg& S = seg[bseg[blockIdx.x]];
    const int64_t i = (int64_t)(blockIdx.x - S.blk0) * blockDim.x + threadIdx.x;
    double d = 0.0, s = 0.0;
    if (i < S.n) {
        const double ai = S.a[i], di = ai - S.o[i];
        d = di * di;
        s = ai * ai;
    }
    d = wsum(d);
    s = wsum(s);
    if ((threadIdx.x & 63) == 0) {
        r1[threadIdx.x >> 6] = d;
        r2[threadIdx.x >> 6] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = (r1[0] + r1[1]) + (r1[2] + r1[3]);
        partial[2 * blockIdx.x + 1] = (r2[0] + r2[1]) + (r2[2] + r2[3]);
    }
}

__global__ void k_reduce_pairs_all(const NormSeg* seg, const double* partial, double* moni) {
    __shared__ double r1[4], r2[4];
    const NormSeg& S = seg[blockIdx.x];
    const double* pp = partial + 2 * S.blk0;
    double d = 0.0, s = 0.0;
    for (int64_t k = threadIdx.x; k < S.nb; k += blockDim.x) {
        d += pp[2 * k];
        s += pp[2 * k + 1];
    }
    d = wsum(d);
    s = wsum(s);
    if ((threadIdx.x & 63) == 0) {
        r1[threadIdx.x >> 6] = d;
        r2[threadIdx.x >> 6] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        moni[S.slot] = (r1[0] + r1[1]) + (r1[2] + r1[3]);
        moni[S.slot + 1] = (r2[0] + r2[1]) + (r2[2] + r2[3]);
    }
}

// ---- interface-eliminated coarse-space correction (MCONTACT.h:2578-2612)
// y[r] = sum_k val[k] W[col[k]] + add[r]: one wavefront per row (coarse rows are long:
// thousands of surface entries each)
__global__ __launch_bounds__(256) void k_csr_wave(const int64_t* ptr, const int32_t* col, const double* val,
                                                  int64_t nrow, const double* W, double* y, const double* add) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= nrow) return;
    const int lane = threadIdx.x & 63;
    double s = 0.0;
    for (int64_t k = ptr[r] + lane; k < ptr[r + 1]; k += 64) s += val[k] * W[col[k]];
    s = wsum(s);
    if (lane == 0) y[r] = add[r] + s;
}

// g[r] = the row's per-source slots in ascending source order (build_coarse)
__global__ void k_slot_sum(const int64_t* sptr, const double* gs, double* g, int64_t n) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    double s = 0.0;
    for (int64_t k = sptr[r]; k < sptr[r + 1]; ++k) s += gs[k];
    g[r] = s;
}

// g[rows[i]] -= yd[src[i]]: the stiffness part of globTran_D_1 u, restricted on the device
__global__ void k_cs_kpart(const int32_t* rows, const int64_t* src, const double* yd, double* g, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) g[rows[i]] -= yd[src[i]];
}

// x[i] = sum_j A[i n + j] g[j]: one wavefront per row of the owned block of globCoup_1^-1
__global__ __launch_bounds__(256) void k_gemv_wave(const double* A, const double* g, double* x, int64_t m, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= m) return;
    const int lane = threadIdx.x & 63;
    const double* a = A + i * n;
    double s = 0.0;
    for (int64_t j = lane; j < n; j += 64) s += a[j] * g[j];
    s = wsum(s);
    if (lane == 0) x[i] = s;
}

// xn = C_d^T xc: nodal level-d values of the owned subdomains (constrained dofs 0)
__global__ void k_cs_scatter(const int32_t* src, const double* xc, double* xn, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) xn[i] = src[i] >= 0 ? xc[src[i]] : 0.0;
}

// u += OUTP_SUB1(accuProl xc): free dofs get (Q (x) I3) xn, constrained dofs their prescribed
// value again (MCONTACT.h:2606-2608 adds OUTP_SUB1's output, Dirichlet values included).
// One thread per batch fine node in the reference order; Q slot-major, <= 8 parents.
__global__ void k_cs_prolong(const int32_t* qcol, const double* qw, int64_t nn, const double* xn, const uint8_t* flag,
                             const double* presc, double* u) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nn) return;
    double e0 = 0.0, e1 = 0.0, e2 = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int32_t c = qcol[(int64_t)k * nn + i];
        if (c < 0) break;
        const double w = qw[(int64_t)k * nn + i];
        e0 += w * xn[c];
        e1 += w * xn[c + 1];
        e2 += w * xn[c + 2];
    }
    const double e[3] = {e0, e1, e2};
    for (int a = 0; a < 3; ++a) {
        const int64_t d = 3 * i + a;
        u[d] += flag[d] ? e[a] : presc[d];
    }
}

// assembled accuProl (operator-level builder): u[tgt[r]] += sum_k val[k] xc[col[k]] over the owned
// subdomains' fine free dofs (one row per thread), then u[cdof[i]] += presc[cdof[i]] on the
// constrained dofs (OUTP_SUB1 writes their prescribed values again, MCONTACT.h:2606-2608)
__global__ void k_cs_prolong_csr(const int64_t* ptr, const int32_t* col, const double* val, const int32_t* tgt,
                                 const double* xc, double* u, int64_t nrow) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrow) return;
    double s = 0.0;
    for (int64_t k = ptr[r]; k < ptr[r + 1]; ++k) s += val[k] * xc[col[k]];
    u[tgt[r]] += s;
}

__global__ void k_cs_presc(const int32_t* cdof, const double* presc, double* u, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) u[cdof[i]] += presc[cdof[i]];
}

// APPS with the DOUBLE_M_1 solve: r = b - A x on the fp64 CSR of globCoup_1 (one wavefront per
// row), and x += d, the refinement step of the Lanczos operator (mcontact_gpu_apps)
__global__ __launch_bounds__(256) void k_apps_resid(const int64_t* ptr, const int32_t* col, const double* val, int64_t nrow,
                                                    const double* x, const double* b, double* r) {
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= nrow) return;
    const int lane = threadIdx.x & 63;
    double s = 0.0;
    for (int64_t k = ptr[i] + lane; k < ptr[i + 1]; k += 64) s += val[k] * x[col[k]];
    s = wsum(s);
    if (lane == 0) r[i] = b[i] - s;
}

__global__ void k_apps_add(double* x, const double* d, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] += d[i];
}

// coarse right-hand side into the coarse MGPIS's fine layout / its solution back to the own rows
__global__ void k_perm_scatter(const int32_t* perm, const double* g, double* b, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) b[perm[i]] = g[i];
}

__global__ void k_perm_gather(const int32_t* perm, const int32_t* rows, const double* x, double* xc, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) xc[i] = x[perm[rows[i]]];
}

// Fused interface update (penalty mass operators proportional to the plain ones, rho = penN =
// penF): with w = M^-1 T^T u and v = M^-1 I gamma from one batched solve,
//   aux = (rho M)^-1 (rho T^T u + M lambda + I gamma) = w + (lambda + v) / rho   (MCONTACT.h:2671-2684)
//   lambda += M^-1 (rho T^T u - rho M aux)             = -v                      (2689-2704)
__global__ void k_fuse_aux_lambda(double* state, const double* wv, const double* rinv, int64_t R) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R) return;
    const double w = wv[i], v = wv[R + i];
    state[i] = w + (state[R + i] + v) * rinv[i];
    state[R + i] = -v;
}

// A planned SELL-64 operator over W (sell_pack, admm_plan.hpp) on the device.
struct SellOp : SellShape {
    DevBuf<int32_t> slots, col;
    DevBuf<int64_t> off;
    DevBuf<double> val;
    void upload(const SellPlan& P) {
        static_cast<SellShape&>(*this) = P;
        slots.upload(P.slots);
        off.upload(P.off);
        col.upload(P.col);
        val.upload(P.val);
    }
    void apply(hipStream_t s, const double* W, double* y, const double* add) const {
        if (nch) hipLaunchKernelGGL(k_sell_w, dim3(ceil_div(nch, 4)), dim3(256), 0, s, slots.p, off.p, col.p, val.p, nch, W, y, add);
    }
};

// DDPCA_STREAMS=1: the batched PCG and the mass CG on one stream each (A/B runs); default two
bool two_streams() {
    const char* v = std::getenv("DDPCA_STREAMS");
    return !(v && v[0] == '1');
}

}  // namespace

// Interface-eliminated coarse space on the device (MCONTACT.h:2578-2612, operators from
// MULTISCALE_1).  Per ADMM iteration, after the subdomain solves:
//   g  = globForc_1 + sum globTran_1 lambda - sum globTran_D_1 u          (2580-2587)
//        globTran_D_1 u = Rc (consStif[L] x) + interface part; the stiffness part is one fp64
//        SpMV of the batch's fine operator followed by the restriction chain to level doleMcsc
//        (factored: Rc consStif[L] would have ~30 entries per fine dof), the rest is one CSR
//        product over the workspace W (columns: owned u and lambda)
//   g summed over ranks (each rank holds the columns it owns), one RCCL all-reduce
//   xc = globCoup_1^-1 g, rows of the owned subdomains (dense inverse from rocSOLVER potrf/potri
//        at setup; the reference factorises with SimplicialLDLT, 2589-2591)
//   u += OUTP_SUB1(accuProl xc)                                             (2600-2610)
struct CoarseDev : CoarseProlongShape {  // (npr, ncd, nxn, qnn, dmin: admm_plan.hpp)
    bool on = false, inverted = false;
    int64_t n = 0, nown = 0;
    double dense_bytes = 0.0;  // n^2 8 B: what the dense inverse would hold per rank
    bool mg_fallback = false;  // (kept for the "coarse_solve" getter: DOUBLE_M is always buildable now)
    DevBuf<double> g, f0, xc, xn, ainv;
    // the right-hand side's per-source slots (build_coarse): rptr/rcol/rval and f0 are per slot,
    // gs the slot values (all-reduced), sptr the slots of each coarse row
    int64_t nslot = 0;
    DevBuf<double> gs;
    DevBuf<int64_t> sptr;
    DevBuf<int64_t> rptr;
    DevBuf<int32_t> rcol;
    DevBuf<double> rval;
    struct KGroup {
        int level = 0;
        DevBuf<int32_t> rows;
        DevBuf<int64_t> src;
    };
    std::vector<KGroup> kg;
    DevBuf<int32_t> xsrc, qcol;
    DevBuf<double> qw;
    DevBuf<uint8_t> flag;
    // assembled variant (cs.assembled): the caller's globTran_D_1 in the right-hand side CSR and
    // accuProl as CSR rows over the owned fine free dofs; factored: the scalar stencil (<= 8
    // parents) for every node it can hold, CSR rows (same arrays) for the rest -- nodes whose chain
    // meets a nodal rotation's 3x3 block (general trees)
    bool assembled = false, latin = false;
    DevBuf<int64_t> pptr;
    DevBuf<int32_t> pcol, ptgt, cdof;
    DevBuf<double> pval;
    std::vector<int64_t> own_rows;  // global coarse rows of this rank, in xc order
    double bytes_iter = 0.0;        // algorithmic bytes of one correction (without DOUBLE_M's PCG)
    // APPS (MCONTACT.h:2343-2403; single-rank, interface-eliminated spaces): the host's globCoup_1
    // and globForc_1, uploaded for the call's true residuals and correlations
    Csr apps_A;
    std::vector<double> apps_f;
    std::vector<double> dense;      // host, until inverted: this rank's rows of globCoup_1 (n x n, zeros elsewhere)
    // DOUBLE_M_1 (MCONTACT.h:2303-2341; the reference's choice once globCoup_1 has DIRE_MAXI rows,
    // 1857-1865): the coarse problem solved by its own MGPIS-PCG, redundantly on every rank, on a
    // hierarchy whose transfers are every subdomain's realProl below doleMcsc, block-diagonal
    bool mg = false;
    bool mg_gather = false;  // a rank-local build: the whole operator is gathered at coarse_invert
    // the coarse MGPIS's structure (plan_coarse_mg, at setup), kept until the operator is there
    // (finish_coarse_mg)
    MgPlan plan;
    Csr gathered_rows;  // this rank's rows of a rank-local operator (sent once at coarse_invert)
    std::unique_ptr<MgpisDevice> cmg;
    DevBuf<int32_t> cperm;  // coarse row -> dof of cmg's fine level (device layout)
    DevBuf<int32_t> cown;   // xc index -> coarse row
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    ~CoarseDev() {
        if (ev_in) (void)hipEventDestroy(ev_in);
        if (ev_out) (void)hipEventDestroy(ev_out);
    }
};

// ================================================================================ handle
// (the workspace layout W = [u (NU) | u on hanging levels (NH) | aux, lambda (2R) | gamma (G)], nsub
// and nint: AdmmLayout; the tables' entries: AdmmSub / AdmmSide / AdmmItf, admm_plan.hpp)
struct ddpca_mcontact : AdmmLayout {
    using Sub = AdmmSub;
    using Side = AdmmSide;
    struct Itf : AdmmItf {
        DevBuf<int32_t> stat;
        DevBuf<double> recv;
    };
    int device = 0, rank = 0, nranks = 1;
    AdmmTuning tune;  // read once at create
    std::vector<int32_t> owner;
    std::vector<Sub> subs;
    std::vector<Side> sides;
    std::vector<Itf> itfs;
    std::unique_ptr<MgpisDevice> mg;
    std::vector<int64_t> maxit;          // per owned subdomain: n_free (reference maxit = rows)
    DevBuf<double> cf;                   // consForc, solver (device) node order
    DevBuf<double> presc;                // Dirichlet values, reference node order (3 nn_L)
    DevBuf<int32_t> onode;               // device node -> reference-order node of the batch
    DevBuf<int32_t> crow;                // coupling rows (solver dofs, surface rows only)
    DevBuf<int64_t> cptr;
    DevBuf<int32_t> ccol;                // columns index W
    DevBuf<double> cval;
    int64_t ncrow = 0;
    DevBuf<double> W;
    SellOp op_hang;                      // hanging-level values: rows of prolOper[maxiLeve] over u
    double* u = nullptr;
    double* state = nullptr;
    double* gamma = nullptr;
    DevBuf<double> uo, state_old, gcst, moni;
    // the MONITOR pair norms as one batch (k_pair_norms_all): segments, block -> segment
    std::vector<NormSeg> norm_seg_host;
    DevBuf<NormSeg> norm_seg;
    DevBuf<int32_t> norm_bseg;
    DevBuf<double> norm_partial;
    SellOp op_gamma, op_aux, op_lam;     // gamma (my halves), aux RHS, lambda RHS
    // rank-local interfaces' side-1 halves (SELL rows; the factored ones in k_gamma_ip), added onto
    // the side-0 halves by k_add_idx: gamma = (constant + half 0) + half 1 on every rank layout
    SellOp op_gamma1;
    DevBuf<double> gam1;
    DevBuf<int32_t> gam1_dst;
    // interfaces whose per-ip operators are applied in factored form (Interface::factored)
    struct FactItf : FactItfShape {
        DevBuf<double> B, M[2], T;
        DevBuf<int32_t> lam[2], u[2];
        DevBuf<int64_t> nptr[2];
        DevBuf<int32_t> niq[2];
        DevBuf<double> ncoef[2];
    };
    std::vector<FactItf> fitfs;
    MassBatch mb_aux, mb_lam;
    // fused interface update (every owned side has inteMass_pena = rho inteMass and
    // systTran_pena = rho systTran): one batched solve of M [w | v] = [T^T u | I gamma]
    bool fused = false;
    SellOp op_wv;
    MassBatch mb_wv;
    DevBuf<double> rinv;
    CoarseDev cs;
    // APPS (mcontact_gpu_apps): the kept Ritz vectors of the last call, n x nev column-major, sign
    // fixed, on the device (mode shapes on demand) and on the host ("apps_vec")
    struct Apps {
        int nev = 0;
        DevBuf<double> Y;
        std::vector<double> Yh;
        double ms[3] = {0.0, 0.0, 0.0};
        double last_solve[2] = {0.0, 0.0};  // DOUBLE_M_1: PCG iterations and recursive ||r|| / ||b|| of the last application
    } apps;
    std::vector<double> moni_host;
    hipStream_t main = nullptr;          // == mg->stream
    std::unique_ptr<Transport> comm;     // RCCL (any rank count, 1 included), or the in-process test transport
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    // reference MONITOR state (MCONTACT.h:2494-2498, 2725-2845)
    int64_t tc = 0;
    int64_t mult_maxi = 1000;  // PREP.h:75 (global in the reference)
    std::vector<std::vector<double>> moniReco;
    std::vector<std::vector<double>> rows;
    double timing[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    double mass_iters = 0.0;
    // algorithmic HBM bytes since the last mcontact_gpu_iterate started (include/ddpca_amd.h,
    // mcontact_gpu_bytes): [0] fine-level PCG kernels, [1] PCG kernels below the fine level + the
    // scalar kernels, [2] coarse-space correction, [3] body-balance RHS + OUTP_SUB1, [4] interface
    // products and projection, [5] batched surface-mass CG, [6] MONITOR snapshot + norms,
    // [7] body-balance PCG launches
    double bytes[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double bytes_rhs = 0.0, bytes_iface = 0.0, bytes_moni = 0.0;  // per ADMM iteration (model, build)
    mgpis_options_t opt{};
};

namespace {

// what the plan sees of the owned subdomains' batch (empty without one)
BatchView batch_view(const MgpisDevice* D) {
    BatchView V;
    if (!D) return V;
    for (const LevelDev& L : D->lev) V.lev.push_back({L.nn, L.noff, L.nloc, L.tent_sub, L.lat});
    V.level_perm = &D->level_perm;
    V.nfree = D->nfree;
    return V;
}

// The handle's device operands from the established problem: each part planned on the host
// (admm_plan.hpp), uploaded, its work buffers allocated, the plan dropped.  Returns the tables for
// build_coarse.
AdmmTables build(ddpca_mcontact& H, const Problem& P) {
    const MCONTACT& mc = P.mc;
    // ---- owned subdomains: one batched MGPIS
    std::vector<AdmmSub> subs = owned_subdomains(P, H.owner, H.rank);
    if (!subs.empty()) {
        std::vector<SubdomainOps> ops;
        for (const auto& S : subs) ops.push_back(subdomain_ops(mc.multGrid[S.tv]));
        H.mg = std::make_unique<MgpisDevice>(H.device, ops, H.opt);
        H.main = H.mg->stream;
        // the body balance's batch on two streams (MgpisDevice::set_split); DDPCA_STREAMS=1 keeps
        // the single-stream graph, DDPCA_PCG_STREAMS=3 / 4 splits it three / four ways (A/B runs)
        const char* ps = std::getenv("DDPCA_PCG_STREAMS");
        H.mg->set_split(two_streams(), ps ? std::max(2, std::min(kMaxParts, std::atoi(ps))) : 2);
    } else {
        DDPCA_HIP(hipStreamCreateWithFlags(&H.main, hipStreamNonBlocking));
    }
    const BatchView V = batch_view(H.mg.get());
    // ---- tables: subdomains, owned sides, interfaces, the regions of W
    AdmmTables T = plan_tables(mc, std::move(subs), H.owner, H.rank, V, H.tune);
    static_cast<AdmmLayout&>(H) = T;
    H.subs = T.subs;
    H.sides = T.sides;
    H.maxit = T.maxit;
    H.cf.upload(T.cf);
    H.presc.upload(T.presc);
    H.onode.upload(T.onode);
    std::vector<double>().swap(T.cf);
    std::vector<double>().swap(T.presc);
    std::vector<int32_t>().swap(T.onode);
    for (const AdmmItf& t : T.itfs) {
        ddpca_mcontact::Itf I;
        static_cast<AdmmItf&>(I) = t;
        if (I.mine) {
            I.stat.alloc(std::max<int64_t>(I.mip / I.comp, 1));
            if (I.cross) I.recv.alloc(I.mip);
        }
        H.itfs.push_back(std::move(I));
    }
    // ---- workspace
    H.W.alloc(H.oG + H.G);
    H.W.zero(H.main);
    H.u = H.W.p;
    H.state = H.W.p + H.oS;
    H.gamma = H.W.p + H.oG;
    H.uo.alloc(H.NU + H.NH);
    H.uo.zero(H.main);
    H.state_old.alloc(std::max<int64_t>(2 * H.R, 2));
    H.state_old.zero(H.main);
    // ---- factored per-ip operators of host-built interfaces this rank handles
    for (const AdmmItf& I : T.itfs) {
        if (!I.mine || !mc.searCont[I.ts].factored) continue;
        const FactItfPlan F = plan_factored(mc, T, I);
        ddpca_mcontact::FactItf D;
        static_cast<FactItfShape&>(D) = F;
        D.B.upload(F.B);
        D.T.alloc(std::max<int64_t>(F.C * F.nip, 1));
        for (int s = 0; s < 2; ++s) {
            if (!F.own[s]) continue;
            D.M[s].upload(F.M[s]);
            D.lam[s].upload(F.lam[s]);
            D.u[s].upload(F.u[s]);
            D.nptr[s].upload(F.nptr[s]);
            D.niq[s].upload(F.niq[s]);
            D.ncoef[s].upload(F.ncoef[s]);
        }
        H.fitfs.push_back(std::move(D));
    }
    // ---- interface operators over W (MCONTACT.h:2632-2636, 2671-2704)
    H.fused = fused_update(mc, T, H.tune);
    {
        const AdmmOperators O = plan_operators(mc, T, H.fused);
        H.op_gamma.upload(O.gamma);
        if (O.has_gamma1) {
            H.op_gamma1.upload(O.gamma1);
            H.gam1.alloc(H.op_gamma1.nrow);
            H.gam1_dst.upload(O.gam1_dst);
        }
        if (!H.fused) {
            H.op_aux.upload(O.aux);
            H.op_lam.upload(O.lam);
        }
        H.gcst.upload(O.gcst);
    }
    // ---- surface-mass batches (built in the fused case too, where mb_wv solves instead: the
    // iteration's check() and byte accounting walk all three batches, and the two cost 0.1 s at
    // the headline size)
    auto build_mass = [&](MassBatch& mb, int which) {
        const MassList L = mass_list(mc, T, which);
        mb.build(L.A, L.roff, L.nrow);
    };
    build_mass(H.mb_aux, 0);
    build_mass(H.mb_lam, 1);
    H.mb_aux.set_split(two_streams());
    H.mb_lam.set_split(two_streams());
    if (H.fused) {
        const AdmmFused F = plan_fused(mc, T);
        H.op_wv.upload(F.wv);
        build_mass(H.mb_wv, 2);
        H.mb_wv.set_split(two_streams());
        H.rinv.upload(F.rinv);
    }
    if (H.tune.verbose)
        std::fprintf(stderr, "[ddpca] interface update: %s\n", H.fused ? "fused (one batched mass solve)" : "sequential");
    // ---- coupling rows of the body-balance RHS
    double coupling_bytes = 0.0;
    {
        const CouplingPlan K = plan_coupling(mc, T, V);
        H.ncrow = (int64_t)K.crow.size();
        coupling_bytes = K.bytes;
        H.crow.upload(K.crow);
        H.cptr.upload(K.cptr);
        H.ccol.upload(K.ccol);
        H.cval.upload(K.cval);
    }
    // ---- hanging-level values over u
    if (H.NH) H.op_hang.upload(plan_hanging(mc, T));
    // ---- per-ADMM-iteration byte model
    {
        std::vector<const FactItfShape*> fact;
        for (const auto& F : H.fitfs) fact.push_back(&F);
        const AdmmBytes B = admm_byte_model(T, H.fused, coupling_bytes, H.op_hang, H.op_gamma, H.op_gamma1, (int64_t)H.gam1_dst.n,
                                            fact, H.op_aux, H.op_lam, H.op_wv);
        H.bytes_rhs = B.rhs;
        H.bytes_iface = B.iface;
        H.bytes_moni = B.moni;
    }
    // monitor norms [2 nsub u | 8 nint aux, lambda | 2 nsub hanging-level parts of u]
    const int64_t nmon = 4 * H.nsub + 8 * H.nint;
    H.moni.alloc(nmon);
    H.moni_host.assign(nmon, 0.0);
    H.moniReco.assign(H.nsub + 4 * H.nint, std::vector<double>(10, 0.0));
    DDPCA_HIP(hipStreamSynchronize(H.main));
    return T;
}

// The coarse MGPIS from the plan and the whole coarse operator A (globCoup_1 / globCoup):
// K[Lc] = A on the hierarchy's fine level, the levels below Galerkin products (MCONTACT.h:
// 1664-1665, 2337-2338)
void finish_coarse_mg(ddpca_mcontact& H, CoarseDev& C, const Csr& A) {
    MgPlan& PL = C.plan;
    const int64_t n = C.n, Lc = (int64_t)PL.nglob.size() - 1;
    if (A.nrow != n || A.ncol != n) throw ApiError(DDPCA_EINVAL, "DOUBLE_M coarse solve: the whole coarse operator is needed");
    std::vector<Bsr3> K(Lc + 1);
    K[Lc] = condensed_to_bsr3(PL.nglob[Lc], n, PL.fdg.data(), A.ptr.data(), A.col.data(), A.val.data());
    for (int64_t l = Lc - 1; l >= 0; --l) K[l] = galerkin_rap(K[l + 1], PL.S[l]);
    SubdomainOps o;
    o.nnodes = PL.nglob;
    for (const auto& k : K) o.K.push_back(&k);
    for (const auto& s : PL.S) o.S.push_back(&s);
    o.dof_free = PL.flev[Lc].data();
    for (const auto& f : PL.flev) o.dof_free_lev.push_back(f.data());
    C.cmg = std::make_unique<MgpisDevice>(H.device, std::vector<SubdomainOps>{o}, H.opt);
    std::vector<int32_t> perm(n), own(C.own_rows.begin(), C.own_rows.end());
    for (int64_t r = 0; r < n; ++r) perm[r] = (int32_t)C.cmg->fine_dof(0, PL.fdg[r]);
    C.cperm.upload(perm);
    C.cown.upload(own.empty() ? std::vector<int32_t>{0} : own);
    DDPCA_HIP(hipEventCreateWithFlags(&C.ev_in, hipEventDisableTiming));
    DDPCA_HIP(hipEventCreateWithFlags(&C.ev_out, hipEventDisableTiming));
    if (H.tune.verbose)
        std::fprintf(stderr, "[ddpca] DOUBLE_M%s coarse solve: %ld rows, %ld levels%s\n", PL.latin ? "" : "_1", (long)n,
                     (long)(Lc + 1), C.mg_gather ? " (operator gathered from every rank)" : "");
    PL = MgPlan();
}

// ---- coarse space: device operands from the host MULTISCALE_1 output (T: build's tables)
void build_coarse(ddpca_mcontact& H, const Problem& P, const AdmmTables& T) {
    const MCONTACT& mc = P.mc;
    const CoarseSpace& cs = mc.coarse;
    CoarseDev& C = H.cs;
    if (!(mc.muscSett & 3)) return;
    if (!cs.ready) throw ApiError(DDPCA_ESTATE, "muscSett set but the coarse space was not built");
    C.on = true;
    C.n = cs.n;
    const int64_t n = C.n;
    // ---- the right-hand side in per-source slots (plan_coarse_rhs has the why)
    CoarseRhsPlan R = plan_coarse_rhs(mc, T);
    C.own_rows = R.own_rows;
    C.nown = (int64_t)C.own_rows.size();
    C.nslot = R.nslot;
    C.bytes_iter = R.bytes;
    C.rptr.upload(R.rptr);
    C.rcol.upload(R.rcol);
    C.rval.upload(R.rval);
    C.sptr.upload(R.slots.sptr);
    C.f0.upload(R.f0);
    std::vector<int64_t>().swap(R.rptr);  // (the slots and xoff stay for the prolongation tables)
    std::vector<int32_t>().swap(R.rcol);
    std::vector<double>().swap(R.rval);
    std::vector<double>().swap(R.f0);
    if (!cs.latin && H.nranks == 1) {
        C.apps_A = cs.globCoup_1;
        C.apps_f.assign(cs.globForc_1.begin(), cs.globForc_1.end());
    }
    C.gs.alloc(std::max<int64_t>(C.nslot, 1));
    C.g.alloc(std::max<int64_t>(n, 1));
    C.xc.alloc(std::max<int64_t>(C.nown, 1));
    // ---- the solve: dense inverse or DOUBLE_M(_1) (coarse_solve_choice)
    const CoarseSolveChoice S = coarse_solve_choice(cs, C.nown, H.nranks, H.tune);
    C.dense_bytes = S.dense_bytes;
    C.mg = S.mg;
    C.mg_gather = S.mg_gather;
    C.latin = cs.latin;
    if (C.mg && H.mg) {
        C.plan = plan_coarse_mg(mc, n);
        if (!C.mg_gather) finish_coarse_mg(H, C, cs.globCoup_1);
        else C.gathered_rows = cs.globCoup_1;  // this rank's rows (its share of the contact rows)
    }
    C.bytes_iter += S.bytes;
    // dense rows of globCoup_1 (inverted once every rank holds all rows)
    if (!C.mg) C.dense = coarse_dense_rows(cs, C.own_rows, H.rank);
    if (!H.mg) return;
    // ---- u += accuProl x_c, and (factored) the stiffness part's gather groups
    C.assembled = cs.assembled;
    if (cs.assembled) {
        const CoarseProlongPlan Q = plan_prolong_assembled(mc, T, R.xoff);
        static_cast<CoarseProlongShape&>(C) = Q;
        C.bytes_iter += Q.bytes;
        C.pptr.upload(Q.pptr);
        C.pcol.upload(Q.pcol);
        C.pval.upload(Q.pval);
        C.ptgt.upload(Q.ptgt);
        C.cdof.upload(Q.cdof);
        return;
    }
    const CoarseProlongPlan Q = plan_prolong_factored(mc, T, batch_view(H.mg.get()), R.slots, R.xoff);
    static_cast<CoarseProlongShape&>(C) = Q;
    for (const KGroupPlan& g : Q.kg) {
        CoarseDev::KGroup G;
        G.level = g.level;
        G.rows.upload(g.rows);
        G.src.upload(g.src);
        C.kg.push_back(std::move(G));
    }
    if (C.npr) {  // the nodes the scalar stencil cannot hold (rotation blocks)
        C.pptr.upload(Q.pptr);
        C.pcol.upload(Q.pcol);
        C.pval.upload(Q.pval);
        C.ptgt.upload(Q.ptgt);
        C.bytes_iter += Q.bytes_csr;
    }
    C.xsrc.upload(Q.xsrc);
    C.xn.alloc(std::max<int64_t>(C.nxn, 1));
    C.qcol.upload(Q.qcol);
    C.qw.upload(Q.qw);
    C.flag.upload(Q.flag);
    C.bytes_iter += Q.bytes;
}

// globCoup_1^-1 rows of the owned subdomains: every rank's rows are summed into a full dense
// copy (one RCCL all-reduce at setup), factorised by rocSOLVER (potrf + potri) on the device
void coarse_invert(ddpca_mcontact& H) {
    CoarseDev& C = H.cs;
    if (!C.on || C.inverted) return;
    if (C.mg) {  // DOUBLE_M: nothing to factorise (the same decision on every rank: n is global)
        if (C.mg_gather) {
            // a rank-local build: every rank's rows (the LATIN contact rows as per-rank shares) as
            // (row, col, value) triplets, all-gathered by two all-reduces (the counts, then each
            // rank's triplets in its own slot); duplicates summed
            if (!H.comm) throw ApiError(DDPCA_ESTATE, "the DOUBLE_M coarse solve of a multi-rank run needs mcontact_gpu_comm_init");
            const Csr& M = C.gathered_rows;
            std::vector<double> cnt(H.nranks, 0.0);
            cnt[H.rank] = (double)M.nnz();
            DevBuf<double> dc;
            dc.upload(cnt);
            H.comm->allreduce_sum(dc.p, H.nranks, H.main);
            DDPCA_HIP(hipStreamSynchronize(H.main));
            cnt = dc.download();
            std::vector<int64_t> off(H.nranks + 1, 0);
            for (int r = 0; r < H.nranks; ++r) off[r + 1] = off[r] + (int64_t)cnt[r];
            std::vector<double> trip(3 * off[H.nranks], 0.0);
            for (int64_t r = 0, q = off[H.rank]; r < M.nrow; ++r)
                for (int64_t k = M.ptr[r]; k < M.ptr[r + 1]; ++k, ++q) {
                    trip[3 * q] = (double)r;
                    trip[3 * q + 1] = (double)M.col[k];
                    trip[3 * q + 2] = M.val[k];
                }
            DevBuf<double> dt;
            dt.upload(trip);
            H.comm->allreduce_sum(dt.p, (int64_t)trip.size(), H.main);
            DDPCA_HIP(hipStreamSynchronize(H.main));
            trip = dt.download();
            const Csr A = triplets_to_csr(trip, off[H.nranks], C.n);
            C.gathered_rows = Csr();
            if (!C.plan.nglob.empty()) finish_coarse_mg(H, C, A);
        }
        C.inverted = true;
        return;
    }
    const int64_t n = C.n;
    if (n > 46000) throw ApiError(DDPCA_EINVAL, "coarse space too large for the dense inverse (n > 46000)");
    DevBuf<double> A;
    A.upload(C.dense);
    std::vector<double>().swap(C.dense);
    hipStream_t st = H.main;
    if (H.nranks > 1 && !H.comm) throw ApiError(DDPCA_ESTATE, "the coarse space of a multi-rank run needs mcontact_gpu_comm_init");
    const bool verbose = H.tune.verbose;
    auto checksum = [n](const std::vector<double>& v) {
        double a = 0.0, b = 0.0;
        for (int64_t i = 0; i < n * n; ++i) a += std::abs(v[i]), b += v[i] * (double)(i % 9973);
        return std::make_pair(a, b);
    };
    if (verbose) {
        const auto c = checksum(A.download());
        std::fprintf(stderr, "[ddpca] rank %d coarse rows %ld owned %ld: own part |.| %.17g w %.17g\n", H.rank, (long)n,
                     (long)C.nown, c.first, c.second);
    }
    if (H.comm) H.comm->allreduce_sum(A.p, n * n, st);
    if (verbose) {
        DDPCA_HIP(hipStreamSynchronize(st));
        const auto c = checksum(A.download());
        std::fprintf(stderr, "[ddpca] rank %d coarse matrix |.| %.17g w %.17g\n", H.rank, c.first, c.second);
    }
    auto solver_guard = solver_lock();
    BlasHandle rh(st);
    DevBuf<rocblas_int> info(2);
    info.zero(st);
    bool accepted;
    if (C.latin) {
        // globCoup (displacements + coarse contact unknowns) is symmetric but indefinite: pivoted
        // LU, then the inverse (symmetric again, so the row-major copy reads it as it is)
        DevBuf<rocblas_int> ipiv(std::max<int64_t>(n, 1));
        accepted = lu_inverse_device(rh, A.p, n, ipiv.p, info.p);
        DDPCA_HIP(hipStreamSynchronize(st));
    } else {
        accepted = spd_inverse_device(rh, A.p, n, info.p);
    }
    C.ainv.alloc(std::max<int64_t>(C.nown, 1) * n);
    // owned rows are contiguous per subdomain (baseReco blocks)
    for (size_t k = 0; k < C.own_rows.size();) {
        size_t e = k;
        while (e + 1 < C.own_rows.size() && C.own_rows[e + 1] == C.own_rows[e] + 1) ++e;
        DDPCA_HIP(hipMemcpyAsync(C.ainv.p + k * n, A.p + C.own_rows[k] * n, (e - k + 1) * n * sizeof(double),
                                 hipMemcpyDeviceToDevice, st));
        k = e + 1;
    }
    DDPCA_HIP(hipStreamSynchronize(st));
    const auto inf = info.download();
    if (!accepted)
        throw ApiError(DDPCA_EHIP, "rocsolver potrf/potri failed on globCoup_1");
    if (inf[0] != 0 || inf[1] != 0)
        throw ApiError(DDPCA_ENUMERIC, std::string(C.latin ? "globCoup is singular (getrf" : "globCoup_1 is not positive definite (potrf") +
                                           " info " + std::to_string(inf[0]) + ")");
    C.inverted = true;
}

// xc = the owned rows of globCoup_1^-1 g, on the stream (the coarse correction's solve and the
// operator of APPS's Lanczos iteration: the same launches).
void coarse_solve(ddpca_mcontact& H, const double* g, double* xc) {
    CoarseDev& C = H.cs;
    hipStream_t st = H.main;
    const int64_t n = C.n;
    if (C.mg) {  // mgpi_1.CG_SOLV(1, globForc, globSolu) (MCONTACT.h:2594), on the coarse solver's stream
        MgpisDevice& M = *C.cmg;
        DDPCA_HIP(hipEventRecord(C.ev_in, st));
        DDPCA_HIP(hipStreamWaitEvent(M.stream, C.ev_in, 0));
        DDPCA_HIP(hipMemsetAsync(M.bs.p, 0, M.bs.n * sizeof(double), M.stream));
        hipLaunchKernelGGL(k_perm_scatter, dim3(nb256(n)), dim3(256), 0, M.stream, C.cperm.p, g, M.bs.p, n);
        M.pcg_solve(1, 1.0e-14, std::vector<int64_t>{n});
        hipLaunchKernelGGL(k_perm_gather, dim3(nb256(C.nown)), dim3(256), 0, M.stream, C.cperm.p, C.cown.p, M.xs.p, xc,
                           C.nown);
        DDPCA_HIP(hipEventRecord(C.ev_out, M.stream));
        DDPCA_HIP(hipStreamWaitEvent(st, C.ev_out, 0));
    } else {
        hipLaunchKernelGGL(k_gemv_wave, dim3(ceil_div(C.nown, 4)), dim3(256), 0, st, C.ainv.p, g, xc, C.nown, n);
    }
}

// u += OUTP_SUB1(accuProl xc) on the owned subdomains (MCONTACT.h:2600-2610): u = the ADMM state,
// or a zeroed scratch of the same layout (APPS's mode shapes, MCONTACT.h:2384-2393)
void coarse_prolong(ddpca_mcontact& H, const double* xc, double* u) {
    CoarseDev& C = H.cs;
    hipStream_t st = H.main;
    if (C.assembled) {
        if (C.npr)
            hipLaunchKernelGGL(k_cs_prolong_csr, dim3(nb256(C.npr)), dim3(256), 0, st, C.pptr.p, C.pcol.p, C.pval.p, C.ptgt.p,
                               xc, u, C.npr);
        if (C.ncd) hipLaunchKernelGGL(k_cs_presc, dim3(nb256(C.ncd)), dim3(256), 0, st, C.cdof.p, H.presc.p, u, C.ncd);
        return;
    }
    hipLaunchKernelGGL(k_cs_scatter, dim3(nb256(C.nxn)), dim3(256), 0, st, C.xsrc.p, xc, C.xn.p, C.nxn);
    hipLaunchKernelGGL(k_cs_prolong, dim3(nb256(C.qnn)), dim3(256), 0, st, C.qcol.p, C.qw.p, C.qnn, C.xn.p, C.flag.p,
                       H.presc.p, u);
    if (C.npr)  // the nodes the scalar stencil cannot hold (rotation blocks)
        hipLaunchKernelGGL(k_cs_prolong_csr, dim3(nb256(C.npr)), dim3(256), 0, st, C.pptr.p, C.pcol.p, C.pval.p, C.ptgt.p,
                           xc, u, C.npr);
}

// One coarse-space correction (MCONTACT.h:2578-2612) on the stream, after k_outp wrote u.
void coarse_correct(ddpca_mcontact& H) {
    CoarseDev& C = H.cs;
    if (!C.inverted) throw ApiError(DDPCA_ESTATE, "coarse space not factorised (multi-rank runs: comm_init first)");
    hipStream_t st = H.main;
    const int64_t n = C.n;
    if (H.mg && !C.assembled) {
        MgpisDevice& D = *H.mg;
        const int L = (int)D.lev.size() - 1;
        // consStif[L] x on every owned subdomain, then realProl^T down to level doleMcsc.  K x is
        // b - r with PCG's recursive residual r: it meets the true one to the PCG accuracy (the
        // reference's own CG_SOLV leaves a true residual of 1e-10 |b| behind its 1e-14 recursive
        // one), and it saves a full fine-level fp64 SpMV per ADMM iteration.  DDPCA_CS_SPMV=1 takes
        // the reference's explicit product instead (consStif * resuSolu, MCONTACT.h:2585-2587);
        // tests/test_headline_gpu.py bounds the difference on the headline option set
        const bool explicit_kx = std::getenv("DDPCA_CS_SPMV") && std::getenv("DDPCA_CS_SPMV")[0] == '1';
        if (explicit_kx) D.spmv(L, D.xs.p, D.lev[L].r.p);
        else
            hipLaunchKernelGGL(k_sub, dim3(nb256(3 * D.lev[L].nn)), dim3(256), 0, st, D.bs.p, D.rs.p, D.lev[L].r.p,
                               3 * D.lev[L].nn);
        for (int l = L; l > C.dmin; --l) D.restrict_level(l, l == L ? D.lev[L].r.p : D.lev[l].b.p, D.lev[l - 1].b.p);
    }
    hipLaunchKernelGGL(k_csr_wave, dim3(std::max(1, ceil_div(C.nslot, 4))), dim3(256), 0, st, C.rptr.p, C.rcol.p,
                       C.rval.p, C.nslot, H.W.p, C.gs.p, C.f0.p);
    if (H.mg && !C.assembled) {
        MgpisDevice& D = *H.mg;
        const int L = (int)D.lev.size() - 1;
        for (auto& G : C.kg) {
            const double* yd = G.level == L ? D.lev[L].r.p : D.lev[G.level].b.p;
            hipLaunchKernelGGL(k_cs_kpart, dim3(nb256(G.rows.n)), dim3(256), 0, st, G.rows.p, G.src.p, yd, C.gs.p,
                               (int64_t)G.rows.n);
        }
    }
    // every slot has one source subdomain, so one rank: the others add exact zeros
    if (H.comm) H.comm->allreduce_sum(C.gs.p, C.nslot, st);
    hipLaunchKernelGGL(k_slot_sum, dim3(nb256(n)), dim3(256), 0, st, C.sptr.p, C.gs.p, C.g.p, n);
    if (!C.nown) return;
    coarse_solve(H, C.g.p, C.xc.p);
    coarse_prolong(H, C.xc.p, H.u);
}

// Reference MONITOR (MCONTACT.h:2725-2845) on the reduced norms; true = converged.
bool monitor(ddpca_mcontact& H) {
    const int64_t cyc = 10;
    const int64_t tc = H.tc;
    const int64_t hb = 2 * H.nsub + 8 * H.nint;  // hanging-level parts of the subdomain norms
    for (int64_t k = 0; k < 2 * H.nsub; ++k) H.moni_host[k] += H.moni_host[hb + k];
    bool flag0 = tc >= cyc, flag1 = true;
    const double c0 = 0.1, c1 = 1.0e-12;
    double convValu = 0.0, convCrit = 0.0;
    std::vector<double> row;
    auto medi_osci = [](const std::vector<double>& v, double& medi, double& osci) {
        const double mx = *std::max_element(v.begin(), v.end()), mn = *std::min_element(v.begin(), v.end());
        medi = (mx + mn) / 2.0;
        osci = mx - mn;
    };
    for (int64_t tv = 0; tv < H.nsub; ++tv) {
        const double d = H.moni_host[2 * tv], a = H.moni_host[2 * tv + 1];
        H.moniReco[tv][tc % cyc] = d;
        convValu += d;
        convCrit += a;
        row.push_back(d);
        row.push_back(a);
        if (tc >= cyc) {
            double me, os;
            medi_osci(H.moniReco[tv], me, os);
            if (os > c0 * me) flag0 = false;
        }
        if (d > c1 * a) flag1 = false;
    }
    for (int64_t ts = 0; ts < H.nint; ++ts)
        for (int s = 0; s < 2; ++s) {
            const double* m = &H.moni_host[2 * H.nsub + 8 * ts + 4 * s];
            const int64_t idx = H.nsub + 4 * ts + 2 * s;
            H.moniReco[idx][tc % cyc] = m[0];
            convValu += m[0];
            convCrit += m[1];
            row.insert(row.end(), {m[0], m[1], m[2], m[3]});
            if (tc >= cyc) {
                double me, os;
                medi_osci(H.moniReco[idx], me, os);
                if (os > c0 * me) flag0 = false;
            }
            if (m[0] > c1 * m[1]) flag1 = false;
            H.moniReco[idx + 1][tc % cyc] = m[2];  // lambda criteria disabled in the reference
        }
    row.push_back(convValu);
    row.push_back(convCrit);
    H.rows.push_back(row);
    if (flag0) H.mult_maxi = tc;
    return flag1;
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

void copy_dev(hipStream_t s, double* y, const double* x, int64_t n) {
    // every copied vector has an even length (3 x multiple of 64, or 2R)
    hipLaunchKernelGGL(k_copy2, dim3(nb256(n / 2)), dim3(256), 0, s, reinterpret_cast<double2*>(y),
                       reinterpret_cast<const double2*>(x), n / 2);
}

// One ADMM iteration; returns true when MONITOR reports convergence.
bool iterate_once(ddpca_mcontact& H, bool check) {
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t st = H.main;
    // snapshot for MONITOR (resuDisp_0 / inteAuxi_0 / inteLagr_0, MCONTACT.h:2507-2509)
    if (H.R) copy_dev(st, H.state_old.p, H.state, 2 * H.R);
    copy_dev(st, H.uo.p, H.u, H.NU + H.NH);
    // ---- body balance: every owned subdomain in one batched PCG
    if (H.mg) {
        MgpisDevice& D = *H.mg;
        copy_dev(st, D.bs.p, H.cf.p, 3 * D.lev.back().nn);
        if (H.ncrow)
            hipLaunchKernelGGL(k_cpl, dim3(nb256(16 * H.ncrow)), dim3(256), 0, st, H.crow.p, H.cptr.p, H.ccol.p, H.cval.p,
                               H.W.p, D.bs.p, H.ncrow);
        D.pcg_begin(1, 1.0e-14, H.maxit, H.opt.warm_start != 0 && H.tc > 0);
        D.pcg_wait(1, 0);
        hipLaunchKernelGGL(k_outp, dim3(nb256(D.lev.back().nn)), dim3(256), 0, st, D.xs.p, D.lev.back().mask.p,
                           H.onode.p, H.presc.p, H.u, D.lev.back().nn);
        if (H.NH) H.op_hang.apply(st, H.W.p, H.W.p + H.oH, nullptr);  // OUTP_SUB1's prolOper[maxiLeve] rows
    }
    // ---- coarse-space correction (MCONTACT.h:2540-2612); OUTP_SUB1 of the correction reaches the
    //      hanging level through the same rows, so they are recomputed from the corrected u
    const bool cs_ran = H.cs.on && H.tc <= H.mult_maxi;
    if (cs_ran) {
        coarse_correct(H);
        if (H.NH) H.op_hang.apply(st, H.W.p, H.W.p + H.oH, nullptr);
    }
    DDPCA_HIP(hipEventRecord(H.ev[1], st));
    const double t_solve = ms_since(t0);
    // ---- interface balance: this rank's gamma halves, one launch for every owned side
    H.op_gamma.apply(st, H.W.p, H.gamma, H.gcst.p);
    if (H.op_gamma1.nch) {
        H.op_gamma1.apply(st, H.W.p, H.gam1.p, nullptr);
        hipLaunchKernelGGL(k_add_idx, dim3(nb256((int64_t)H.gam1_dst.n)), dim3(256), 0, st, H.gamma, H.gam1.p, H.gam1_dst.p,
                           (int64_t)H.gam1_dst.n);
    }
    for (auto& F : H.fitfs) {
        const IpSide s0{F.M[0].p, F.lam[0].p, F.u[0].p}, s1{F.M[1].p, F.lam[1].p, F.u[1].p};
        if (F.nip)
            hipLaunchKernelGGL(k_gamma_ip, dim3(nb256(F.nip)), dim3(256), 0, st, F.B.p, s0, s1, F.own[0], F.own[1], F.pen[0],
                               F.pen[1], F.pen[2], F.C, F.nip, H.W.p, H.gamma + F.goff, H.gcst.p + F.goff);
    }
    bool any_cross = false;
    for (auto& I : H.itfs) any_cross |= (I.cross && I.mine);
    DDPCA_HIP(hipEventRecord(H.ev[0], st));
    if (any_cross) {
        if (!H.comm) throw ApiError(DDPCA_ESTATE, "cross-rank interfaces need mcontact_gpu_comm_init");
        std::vector<Transport::Msg> msgs;
        for (auto& I : H.itfs) {
            if (!(I.cross && I.mine)) continue;
            const int peer = I.owner[0] == H.rank ? I.owner[1] : I.owner[0];
            msgs.push_back({peer, I.ts, H.gamma + I.goff, I.recv.p, I.mip});
        }
        H.comm->exchange(msgs, st);
        for (auto& I : H.itfs)
            if (I.cross && I.mine)
                hipLaunchKernelGGL(k_add, dim3(nb256(I.mip)), dim3(256), 0, st, H.gamma + I.goff, I.recv.p, I.mip);
    }
    DDPCA_HIP(hipEventRecord(H.ev[2], st));
    for (auto& I : H.itfs)
        if (I.mine)
            hipLaunchKernelGGL(k_project, dim3(nb256(I.mip / I.comp)), dim3(256), 0, st, H.gamma + I.goff, I.stat.p,
                               I.mip / I.comp, I.comp, I.fric);
    // ---- aux = (M^rho)^-1 (T^T u + M lambda + I gamma), lambda += M^-1 (T^T u - M^rho aux)
    if (H.fused) {
        H.op_wv.apply(st, H.W.p, H.mb_wv.b.p, nullptr);
        for (auto& F : H.fitfs) {  // the inteInpo gamma half of the factored interfaces
            if (!F.nip) continue;
            hipLaunchKernelGGL(k_traction_ip, dim3(nb256(F.nip)), dim3(256), 0, st, F.B.p, H.gamma + F.goff, F.T.p, F.C,
                               F.nip);
            for (int s = 0; s < 2; ++s)
                if (F.own[s] && F.nnc[s])
                    hipLaunchKernelGGL(k_inpo_node, dim3(ceil_div(F.nnc[s], 4)), dim3(256), 0, st, F.nptr[s].p, F.niq[s].p,
                                       F.ncoef[s].p, F.T.p, F.C, F.nnc[s], H.mb_wv.b.p + H.R + F.roff[s]);
        }
        H.mb_wv.solve(st, H.mb_wv.x.p, 1.0e-14, 2000);
        hipLaunchKernelGGL(k_fuse_aux_lambda, dim3(nb256(H.R)), dim3(256), 0, st, H.state, H.mb_wv.x.p, H.rinv.p, H.R);
    } else if (!H.sides.empty()) {
        H.op_aux.apply(st, H.W.p, H.mb_aux.b.p, nullptr);
        H.mb_aux.solve(st, H.state, 1.0e-14, 2000);
        // ---- lambda += M^-1 (T^T u - M^rho aux)
        H.op_lam.apply(st, H.W.p, H.mb_lam.b.p, nullptr);
        H.mb_lam.solve(st, H.mb_lam.x.p, 1.0e-14, 2000);
        hipLaunchKernelGGL(k_add, dim3(nb256(H.R)), dim3(256), 0, st, H.state + H.R, H.mb_lam.x.p, H.R);
    }
    // ---- MONITOR norms (owned entries; others zero) and their reduction across ranks
    DDPCA_HIP(hipMemsetAsync(H.moni.p, 0, H.moni.n * sizeof(double), st));
    {
        std::vector<NormSeg> seg;
        int64_t nblk = 0;
        auto add = [&](const double* a, const double* o, int64_t n, int64_t slot) {
            const int64_t nb = nb256(n);
            seg.push_back({a, o, n, nblk, nb, slot});
            nblk += nb;
        };
        for (auto& S : H.subs) {
            add(H.u + S.dof0, H.uo.p + S.dof0, 3 * S.nn, 2 * S.tv);
            if (S.nh) add(H.u + H.oH + S.hoff, H.uo.p + H.oH + S.hoff, S.nh, 2 * H.nsub + 8 * H.nint + 2 * S.tv);
        }
        for (auto& sd : H.sides) {
            const int64_t base = 2 * H.nsub + 8 * sd.ts + 4 * sd.s;
            add(H.state + sd.roff, H.state_old.p + sd.roff, sd.m, base);
            add(H.state + H.R + sd.roff, H.state_old.p + H.R + sd.roff, sd.m, base + 2);
        }
        if (!seg.empty()) {
            // the segments are the same every iteration: upload once (and again if they change)
            const bool same = seg.size() == H.norm_seg_host.size() &&
                              std::memcmp(seg.data(), H.norm_seg_host.data(), seg.size() * sizeof(NormSeg)) == 0;
            if (!same) {
                std::vector<int32_t> bseg(nblk);
                for (size_t g = 0; g < seg.size(); ++g)
                    for (int64_t k = 0; k < seg[g].nb; ++k) bseg[seg[g].blk0 + k] = (int32_t)g;
                DDPCA_HIP(hipStreamSynchronize(st));  // the previous iteration's launches read the old table
                H.norm_seg.upload(seg);
                H.norm_bseg.upload(bseg);
                H.norm_partial.alloc(2 * nblk);
                H.norm_seg_host = seg;
            }
            hipLaunchKernelGGL(k_pair_norms_all, dim3((unsigned)nblk), dim3(256), 0, st, H.norm_seg.p, H.norm_bseg.p,
                               H.norm_partial.p);
            hipLaunchKernelGGL(k_reduce_pairs_all, dim3((unsigned)seg.size()), dim3(256), 0, st, H.norm_seg.p,
                               H.norm_partial.p, H.moni.p);
        }
    }
    if (H.comm) H.comm->allreduce_sum(H.moni.p, H.moni.n, st);
    DDPCA_HIP(hipEventRecord(H.ev[3], st));
    DDPCA_HIP(hipMemcpyAsync(H.moni_host.data(), H.moni.p, H.moni.n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (H.mg) H.mg->pcg_fetch();
    DDPCA_HIP(hipStreamSynchronize(st));
    if (H.mg) H.mg->pcg_check();
    H.mb_aux.check();
    H.mb_lam.check();
    H.mb_wv.check();
    float a = 0, b = 0;
    (void)hipEventElapsedTime(&a, H.ev[1], H.ev[3]);
    (void)hipEventElapsedTime(&b, H.ev[0], H.ev[2]);
    H.timing[0] += ms_since(t0);
    H.timing[1] += t_solve;
    H.timing[2] += a;
    H.timing[3] += any_cross ? b : 0.0;
    H.mass_iters += (double)(H.fused ? H.mb_wv.last_iters : H.mb_aux.last_iters + H.mb_lam.last_iters);
    if (H.mg) {
        MgpisDevice& D = *H.mg;
        for (int s = 0; s < D.nsub; ++s) {
            H.timing[6] += (double)D.sc_host[s].iter;
            H.timing[8] += (double)D.sc_host[s].iter * (double)D.nfree[s];
        }
        if (D.timed_kernel_samples) {
            H.timing[7] += D.timed_kernel_bytes;
            H.timing[4] += D.timed_kernel_ms;
            H.timing[5] += (double)D.timed_kernel_samples;
            D.timed_kernel_ms = 0.0;
            D.timed_kernel_bytes = 0.0;
            D.timed_kernel_samples = 0;
        }
    }
    if (H.mg) {
        MgpisDevice& D = *H.mg;
        H.bytes[0] += D.alg_bytes[0];
        H.bytes[1] += D.alg_bytes[1];
        H.bytes[7] += D.alg_bytes[2];
        D.alg_bytes[0] = D.alg_bytes[1] = D.alg_bytes[2] = 0.0;
    }
    if (cs_ran) {
        H.bytes[2] += H.cs.bytes_iter;
        if (H.cs.cmg) {
            H.bytes[2] += H.cs.cmg->alg_bytes[0] + H.cs.cmg->alg_bytes[1];
            H.cs.cmg->alg_bytes[0] = H.cs.cmg->alg_bytes[1] = H.cs.cmg->alg_bytes[2] = 0.0;
        }
    }
    H.bytes[3] += H.bytes_rhs;
    H.bytes[4] += H.bytes_iface;
    for (MassBatch* mb : {&H.mb_aux, &H.mb_lam, &H.mb_wv}) {
        H.bytes[5] += mb->alg_bytes;
        mb->alg_bytes = 0.0;
    }
    H.bytes[6] += H.bytes_moni;
    const bool conv = monitor(H);
    H.tc += 1;
    return check && conv;
}

}  // namespace

// resuDisp of an owned subdomain where it lives in the workspace (mcontact_gpu_stress,
// capi_stress.hip): the fine level's dofs, then the hanging level's (mcontact_gpu_get "resuDisp")
namespace ddpca {
bool mcontact_sub_disp(mcontact_t h, int64_t tv, SubDisp* out) {
    for (const auto& S : h->subs)
        if (S.tv == tv) {
            out->device = h->device;
            out->stream = h->main;
            out->u_main = h->u + S.dof0;
            out->u_hang = h->u + h->oH + S.hoff;
            out->nn = S.nn;
            out->nh = S.nh;
            return true;
        }
    return false;
}
}  // namespace ddpca

extern "C" {

// Every graph the ADMM iteration replays, captured on the calling thread (create, or after the
// in-process ranks' setup threads joined): a capture running on one rank thread was invalidated
// by another rank thread's synchronous HIP calls in the in-process multi-rank runs.
// Idempotent: what exists is kept.
void prepare_graphs(ddpca_mcontact& H) {
    if (H.mg) H.mg->prepare_graphs(1);
    if (H.fused) H.mb_wv.prepare(H.main, H.mb_wv.x.p);
    else if (!H.sides.empty()) {
        H.mb_aux.prepare(H.main, H.state);
        H.mb_lam.prepare(H.main, H.mb_lam.x.p);
    }
    if (H.cs.cmg) H.cs.cmg->prepare_graphs(1);
    DDPCA_HIP(hipStreamSynchronize(H.main));
}

int mcontact_gpu_create(ddpca_problem_t p, int device, int rank, int nranks, const int32_t* owner,
                        const mgpis_options_t* opt, mcontact_t* out) {
    return guarded([&] {
        Problem& P = *reinterpret_cast<Problem*>(p);
        if (!P.established) throw ApiError(DDPCA_ESTATE, "problem not established");
        if (nranks < 1 || rank < 0 || rank >= nranks || !owner || !out) throw ApiError(DDPCA_EINVAL, "rank/owner");
        select_device(device);
        auto H = std::make_unique<ddpca_mcontact>();
        H->device = device;
        H->rank = rank;
        H->nranks = nranks;
        H->owner.assign(owner, owner + P.mc.multGrid.size());
        for (int32_t o : H->owner)
            if (o < 0 || o >= nranks) throw ApiError(DDPCA_EINVAL, "owner out of range");
        if (opt) H->opt = *opt;
        else mgpis_default_options(&H->opt);
        for (auto& e : H->ev) DDPCA_HIP(hipEventCreate(&e));
        H->tune = admm_tuning();
        const AdmmTables T = build(*H, P);
        build_coarse(*H, P, T);
        if (nranks == 1) coarse_invert(*H);
        prepare_graphs(*H);
        *out = H.release();
    });
}

int mcontact_gpu_unique_id(void* out128) {
    return guarded([&] { rccl_unique_id(out128); });
}

int mcontact_gpu_comm_init(mcontact_t h, const void* uid) {
    return guarded([&] {
        if (!h || !uid) throw ApiError(DDPCA_EINVAL, "handle / unique id");
        select_device(h->device);
        if (h->comm) throw ApiError(DDPCA_ESTATE, "handle already has a communicator");
        // nranks == 1 builds a one-rank communicator too: the MONITOR and coarse-RHS all-reduces then
        // run through RCCL on the solve stream (bit-identical to the run without one)
        h->comm = rccl_transport(h->nranks, h->rank, uid);
        coarse_invert(*h);
        prepare_graphs(*h);
    });
}

int mcontact_gpu_comm_local(mcontact_t* handles, int n) {
    return guarded([&] {
        if (!handles || n < 1) throw ApiError(DDPCA_EINVAL, "handles");
        for (int r = 0; r < n; ++r) {
            if (!handles[r] || handles[r]->nranks != n || handles[r]->rank != r)
                throw ApiError(DDPCA_EINVAL, "handles[r] must be rank r of n");
            if (handles[r]->comm) throw ApiError(DDPCA_ESTATE, "handle already has a communicator");
        }
        auto ts = local_transports(n);
        for (int r = 0; r < n; ++r) handles[r]->comm = std::move(ts[r]);
        // the setup all-reduce of the coarse matrix is collective: one host thread per rank
        std::vector<std::thread> th;
        std::vector<int> rc(n, 0);
        std::vector<std::string> msg(n);
        for (int r = 0; r < n; ++r)
            th.emplace_back([&, r] {
                rc[r] = guarded([&] {
                    select_device(handles[r]->device);
                    coarse_invert(*handles[r]);
                });
                if (rc[r] < 0) msg[r] = ddpca_last_error();
            });
        for (auto& t : th) t.join();
        for (int r = 0; r < n; ++r)
            if (rc[r] < 0) throw ApiError(rc[r], "rank " + std::to_string(r) + ": " + msg[r]);
        for (int r = 0; r < n; ++r) {  // the gathered DOUBLE_M solvers' graphs, one rank at a time
            select_device(handles[r]->device);
            prepare_graphs(*handles[r]);
        }
    });
}

int mcontact_gpu_comm_loopback(mcontact_t h, ddpca_problem_t p) {
    return guarded([&] {
        if (!h || !p) throw ApiError(DDPCA_EINVAL, "handle / problem");
        select_device(h->device);
        if (h->comm) throw ApiError(DDPCA_ESTATE, "handle already has a communicator");
        CoarseDev& C = h->cs;
        // a rank-local DOUBLE_M operator would be "gathered" through the identity all-reduce: this
        // rank's rows only, a singular coarse hierarchy
        if (C.on && !C.inverted && C.mg_gather)
            throw ApiError(DDPCA_ESTATE, "loopback: the problem must be the handle's, established in full "
                                         "(a rank-local DOUBLE_M coarse operator cannot be gathered)");
        h->comm = loopback_transport();
        if (C.on && !C.inverted && !C.mg) {
            // the other ranks' rows of the dense coarse operator come from the problem itself (the
            // setup all-reduce that would sum them is the identity here)
            const CoarseSpace& cs = reinterpret_cast<Problem*>(p)->mc.coarse;
            if (cs.rank_local || cs.n != C.n)
                throw ApiError(DDPCA_ESTATE, "loopback: the problem must be the handle's, established in full");
            const int64_t n = C.n;
            C.dense.assign((size_t)n * n, 0.0);
            for (int64_t r = 0; r < n; ++r)
                for (int64_t k = cs.globCoup_1.ptr[r]; k < cs.globCoup_1.ptr[r + 1]; ++k)
                    C.dense[(size_t)r * n + cs.globCoup_1.col[k]] = cs.globCoup_1.val[k];
        }
        coarse_invert(*h);
        prepare_graphs(*h);
    });
}

int mcontact_gpu_comm_check(mcontact_t h, int64_t n) {
    return guarded([&] {
        if (!h || n < 1) throw ApiError(DDPCA_EINVAL, "handle / n");
        select_device(h->device);
        if (!h->comm) throw ApiError(DDPCA_ESTATE, "no communicator (mcontact_gpu_comm_init / _comm_local)");
        const int R = h->nranks, me = h->rank;
        hipStream_t st = h->main;
        // exchange: to every rank q (me included) two messages, tagged by the unordered pair {me, q}
        // and k as the interfaces' gamma halves are (both ends name the same tag);
        // message (me -> q, k) carries v = 1e6 me + 1e3 q + k + i 2^-20 (exact in fp64)
        auto val = [](int src, int dst, int k, int64_t i) { return 1.0e6 * src + 1.0e3 * dst + k + std::ldexp((double)i, -20); };
        std::vector<double> hs((size_t)R * 2 * n);
        for (int q = 0; q < R; ++q)
            for (int k = 0; k < 2; ++k)
                for (int64_t i = 0; i < n; ++i) hs[((size_t)q * 2 + k) * n + i] = val(me, q, k, i);
        DevBuf<double> sbuf, rbuf((size_t)R * 2 * n), ar(n);
        sbuf.upload(hs);
        std::vector<Transport::Msg> msgs;
        for (int q = 0; q < R; ++q)
            for (int k = 0; k < 2; ++k)
                msgs.push_back({q, 2 * ((int64_t)std::min(me, q) * R + std::max(me, q)) + k, sbuf.p + ((size_t)q * 2 + k) * n, rbuf.p + ((size_t)q * 2 + k) * n, n});
        h->comm->exchange(msgs, st);
        // all-reduce: rank r contributes (r + 1) (i + 1); the sum is R (R + 1) / 2 (i + 1)
        std::vector<double> ha(n);
        for (int64_t i = 0; i < n; ++i) ha[i] = (double)(me + 1) * (double)(i + 1);
        DDPCA_HIP(hipMemcpyAsync(ar.p, ha.data(), n * sizeof(double), hipMemcpyHostToDevice, st));
        h->comm->allreduce_sum(ar.p, n, st);
        DDPCA_HIP(hipStreamSynchronize(st));
        const auto hr = rbuf.download();
        const auto hsum = ar.download();
        for (int q = 0; q < R; ++q)
            for (int k = 0; k < 2; ++k)
                for (int64_t i = 0; i < n; ++i)
                    if (hr[((size_t)q * 2 + k) * n + i] != val(q, me, k, i))
                        throw ApiError(DDPCA_ECOMM, "comm check: message " + std::to_string(k) + " from rank " + std::to_string(q) +
                                                        " arrived wrong at element " + std::to_string(i));
        for (int64_t i = 0; i < n; ++i)
            if (hsum[i] != 0.5 * R * (R + 1) * (double)(i + 1))
                throw ApiError(DDPCA_ECOMM, "comm check: all-reduce element " + std::to_string(i) + " wrong");
    });
}

int64_t mcontact_gpu_iterate(mcontact_t h, int64_t maxit, int check) {
    int64_t n = 0;
    const int rc = guarded([&] {
        select_device(h->device);
        for (double& t : h->timing) t = 0.0;
        for (double& b : h->bytes) b = 0.0;
        h->mass_iters = 0.0;
        if (h->mg) h->mg->time_kernel = true;
        if (h->nranks > 1 && !h->comm) throw ApiError(DDPCA_ESTATE, "a multi-rank run needs mcontact_gpu_comm_init");
        for (; n < maxit;) {
            const bool conv = iterate_once(*h, check != 0);
            ++n;
            if (conv) break;
        }
    });
    return rc < 0 ? rc : n;
}

int64_t mcontact_gpu_monitor(mcontact_t h, double* out, int64_t cap_rows) {
    const int64_t rows = (int64_t)h->rows.size();
    if (!out) return rows;
    const int64_t ncol = 2 * h->nsub + 8 * h->nint + 2;
    for (int64_t r = 0; r < std::min(rows, cap_rows); ++r) std::memcpy(out + r * ncol, h->rows[r].data(), ncol * sizeof(double));
    return std::min(rows, cap_rows);
}

int64_t mcontact_gpu_get(mcontact_t h, const char* what, int64_t index, void* out, int64_t cap) {
    int64_t n = 0;
    const int rc = guarded([&] {
        select_device(h->device);
        const std::string w(what);
        DDPCA_HIP(hipStreamSynchronize(h->main));
        if (w == "resuDisp") {
            for (auto& S : h->subs)
                if (S.tv == index) {  // position numbering: level-maxiLeve nodes, then the hanging level
                    n = 3 * S.nn + S.nh;
                    if (out) {
                        DDPCA_HIP(hipMemcpy(out, h->u + S.dof0, std::min(3 * S.nn, cap) * sizeof(double), hipMemcpyDeviceToHost));
                        if (cap > 3 * S.nn && S.nh)
                            DDPCA_HIP(hipMemcpy(static_cast<double*>(out) + 3 * S.nn, h->u + h->oH + S.hoff,
                                                std::min(S.nh, cap - 3 * S.nn) * sizeof(double), hipMemcpyDeviceToHost));
                    }
                    return;
                }
            throw ApiError(DDPCA_EINVAL, "subdomain not owned by this rank");
        }
        if (w == "inteAuxi" || w == "inteLagr") {
            for (auto& sd : h->sides)
                if (2 * sd.ts + sd.s == index) {
                    n = sd.m;
                    const double* src = h->state + sd.roff + (w == "inteAuxi" ? 0 : h->R);
                    if (out) DDPCA_HIP(hipMemcpy(out, src, std::min(n, cap) * sizeof(double), hipMemcpyDeviceToHost));
                    return;
                }
            throw ApiError(DDPCA_EINVAL, "interface side not owned by this rank");
        }
        if (w == "inpoGamm") {
            for (auto& I : h->itfs)
                if (I.ts == index && I.mine) {
                    n = I.mip;
                    if (out) DDPCA_HIP(hipMemcpy(out, h->gamma + I.goff, std::min(n, cap) * sizeof(double), hipMemcpyDeviceToHost));
                    return;
                }
            throw ApiError(DDPCA_EINVAL, "interface not handled by this rank");
        }
        if (w == "fricStat") {
            for (auto& I : h->itfs)
                if (I.ts == index && I.mine) {
                    n = I.mip / I.comp;
                    if (out) DDPCA_HIP(hipMemcpy(out, I.stat.p, std::min(n, cap) * sizeof(int32_t), hipMemcpyDeviceToHost));
                    return;
                }
            throw ApiError(DDPCA_EINVAL, "interface not handled by this rank");
        }
        if (w == "pcg_iters") {
            n = (int64_t)h->subs.size();
            if (out)
                for (int64_t i = 0; i < std::min(n, cap); ++i) static_cast<int64_t*>(out)[i] = h->mg->sc_host[i].iter;
            return;
        }
        if (w == "owned") {
            n = (int64_t)h->subs.size();
            if (out)
                for (int64_t i = 0; i < std::min(n, cap); ++i) static_cast<int64_t*>(out)[i] = h->subs[i].tv;
            return;
        }
        if (w == "coarse_solve") {
            // [rows, 1 = multigrid (DOUBLE_M / DOUBLE_M_1) else 0, dense inverse bytes,
            //  1 = the budget asked for DOUBLE_M but its hierarchy was not buildable (dense kept)]
            n = 4;
            if (out && cap >= 4) {
                auto* o = static_cast<int64_t*>(out);
                o[0] = h->cs.on ? h->cs.n : 0;
                o[1] = h->cs.on && h->cs.mg ? 1 : 0;
                o[2] = h->cs.on && !h->cs.mg ? (int64_t)h->cs.dense_bytes : 0;
                o[3] = h->cs.mg_fallback ? 1 : 0;
            }
            return;
        }
        if (w == "mass_iters") {
            n = 1;
            if (out && cap >= 1) static_cast<int64_t*>(out)[0] = (int64_t)h->mass_iters;
            return;
        }
        if (w == "gs_rows") {  // int64 [rows the colour sweeps cover, ring rows, far rows] (GsFine::band)
            int64_t v[3] = {0, 0, 0};
            if (h->mg && h->mg->gs_fine()) {
                const GsFine& G = h->mg->gs;
                for (int s = 0; s < h->mg->nsub; ++s) {
                    v[0] += G.band ? G.band_rows_sub[s] : h->mg->lev.back().nloc[s];
                    v[1] += G.band ? G.ring_rows_sub[s] : 0;
                    v[2] += G.band ? G.far_rows_sub[s] : 0;
                }
            }
            n = 3;
            if (out)
                for (int64_t i = 0; i < std::min<int64_t>(3, cap); ++i) static_cast<int64_t*>(out)[i] = v[i];
            return;
        }
        if (w == "gs_launch_bytes") {  // the colour sweeps' per-launch byte model (GsFine::launch_bytes), doubles
            if (!h->mg) throw ApiError(DDPCA_ESTATE, "no owned subdomain");
            const auto& v = h->mg->gs.launch_bytes;
            n = (int64_t)v.size();
            if (out)
                for (int64_t i = 0; i < std::min(n, cap); ++i) static_cast<double*>(out)[i] = v[i];
            return;
        }
        if (w == "apps_vec") {  // coarse eigenvector y_index of the last mcontact_gpu_apps (n doubles, unit norm)
            if (h->apps.nev < 1) throw ApiError(DDPCA_ESTATE, "no mcontact_gpu_apps result");
            if (index < 0 || index >= h->apps.nev) throw ApiError(DDPCA_EINVAL, "mode index out of range");
            n = h->cs.n;
            if (out) std::memcpy(out, h->apps.Yh.data() + index * n, std::min(n, cap) * sizeof(double));
            return;
        }
        if (w == "apps_timing") {
            // doubles: ms of the operator applications, the orthogonalisation, the Ritz products
            // (DDPCA_APPS_TIMING=1, else 0); DOUBLE_M_1's last application: PCG iterations, recursive ||r|| / ||b||
            const double v[5] = {h->apps.ms[0], h->apps.ms[1], h->apps.ms[2], h->apps.last_solve[0], h->apps.last_solve[1]};
            n = 5;
            if (out)
                for (int64_t i = 0; i < std::min<int64_t>(5, cap); ++i) static_cast<double*>(out)[i] = v[i];
            return;
        }
        throw ApiError(DDPCA_EINVAL, "unknown quantity " + w);
    });
    return rc < 0 ? rc : n;
}

int mcontact_gpu_timing(mcontact_t h, double* out10) {
    std::memcpy(out10, h->timing, sizeof(h->timing));
    if (h->timing[5] > 0) out10[7] = h->timing[7] / h->timing[5];  // bytes per timed launch
    double dofs = 0.0;
    if (h->mg)
        for (int64_t nf : h->mg->nfree) dofs += (double)nf;
    out10[9] = dofs;
    return DDPCA_OK;
}

int64_t mcontact_gpu_bytes(mcontact_t h, double* out, int64_t cap) {
    const int64_t n = (int64_t)(sizeof(h->bytes) / sizeof(double));
    if (out)
        for (int64_t i = 0; i < std::min(n, cap); ++i) out[i] = h->bytes[i];
    return n;
}

// MCONTACT::APPS (MCONTACT.h:2343-2403): the nev eigenpairs of smallest magnitude of globCoup_1 by
// thick-restart Lanczos on its device-resident inverse (device_eigs.hip), each mode's correlation
// with the coarse load.  Touches nothing of the ADMM state: the basis and the Ritz vectors are
// the call's own, the coarse solve's right-hand side and result are columns of that basis.
int mcontact_gpu_apps(mcontact_t h, int64_t nev, int64_t ncv, double tol, int64_t max_restarts, double* eigval,
                      double* corr, double* resid, int64_t* info) {
    return guarded([&] {
        if (!h) throw ApiError(DDPCA_EINVAL, "mcontact_gpu_apps: NULL handle");
        if (h->nranks > 1)
            throw ApiError(DDPCA_EINVAL, "mcontact_gpu_apps: a rank of a multi-rank run holds only its own rows of "
                                         "globCoup_1^-1 (the distributed eigen-solver is not implemented)");
        CoarseDev& C = h->cs;
        if (!C.on || C.latin)
            throw ApiError(DDPCA_ESTATE, "mcontact_gpu_apps: no interface-eliminated coarse space (muscSett = 2): globCoup_1 is empty");
        if (!C.inverted || !h->mg) throw ApiError(DDPCA_ESTATE, "mcontact_gpu_apps: coarse space not factorised");
        const int64_t n = C.n;
        if (C.nown != n || C.apps_A.nrow != n || (int64_t)C.apps_f.size() != n)
            throw ApiError(DDPCA_ESTATE, "mcontact_gpu_apps: the handle does not hold every row of globCoup_1");
        if (ncv == 0) ncv = std::min<int64_t>(20 * nev, n);  // the reference's ncv (MCONTACT.h:2354)
        if (tol == 0.0) tol = 1.0e-6;                        // and its tolerance (2358)
        if (nev < 1 || ncv <= nev || ncv > n)
            throw ApiError(DDPCA_EINVAL, "mcontact_gpu_apps: need 1 <= nev < ncv <= n (n = " + std::to_string(n) + ")");
        if (ncv > kEigsMaxNcv)
            throw ApiError(DDPCA_EINVAL, "mcontact_gpu_apps: ncv above " + std::to_string(kEigsMaxNcv));
        if (!(tol > 0.0) || max_restarts < 0 || !eigval || !corr || !resid)
            throw ApiError(DDPCA_EINVAL, "mcontact_gpu_apps: tol, max_restarts or a NULL output");
        select_device(h->device);
        hipStream_t st = h->main;
        DDPCA_HIP(hipStreamSynchronize(st));
        DevBuf<int64_t> aptr;
        DevBuf<int32_t> acol;
        DevBuf<double> aval;
        aptr.upload(C.apps_A.ptr);
        acol.upload(C.apps_A.col.empty() ? std::vector<int32_t>{0} : C.apps_A.col);
        aval.upload(C.apps_A.val.empty() ? std::vector<double>{0.0} : C.apps_A.val);
        h->apps.nev = 0;
        h->apps.Y.alloc((size_t)n * nev);
        // the coarse MGPIS's measurement counters belong to the ADMM iterations
        double keep_bytes[3] = {0, 0, 0}, keep_ms = 0.0, keep_tb = 0.0;
        int64_t keep_samples = 0, keep_graphs = 0;
        if (C.cmg) {
            std::memcpy(keep_bytes, C.cmg->alg_bytes, sizeof(keep_bytes));
            keep_ms = C.cmg->timed_kernel_ms, keep_tb = C.cmg->timed_kernel_bytes;
            keep_samples = C.cmg->timed_kernel_samples, keep_graphs = C.cmg->graphs_launched;
        }
        auto restore = [&] {
            if (!C.cmg) return;
            std::memcpy(C.cmg->alg_bytes, keep_bytes, sizeof(keep_bytes));
            C.cmg->timed_kernel_ms = keep_ms, C.cmg->timed_kernel_bytes = keep_tb;
            C.cmg->timed_kernel_samples = keep_samples, C.cmg->graphs_launched = keep_graphs;
        };
        DevBuf<double> rres(C.mg ? n : 0), rcor(C.mg ? n : 0);
        EigsResult R;
        const char* tenv = std::getenv("DDPCA_APPS_TIMING");
        try {
            // DOUBLE_M_1's PCG stops on its recursive residual; its true residual is amplified by
            // kappa(A) on the lowest modes (2e-7 measured on beam_dd_m2, kappa = 4.8e6) and is the
            // floor of the eigen-residual.  One refinement step on the true residual removes it:
            // y = S b, y += S (b - A y), S the coarse correction's solve both times
            auto op = [&](const double* x, double* y) {
                coarse_solve(*h, x, y);
                if (!C.mg) return;
                hipLaunchKernelGGL(k_apps_resid, dim3(ceil_div(n, 4)), dim3(256), 0, st, aptr.p, acol.p, aval.p, n, y, x, rres.p);
                coarse_solve(*h, rres.p, rcor.p);
                hipLaunchKernelGGL(k_apps_add, dim3(nb256(n)), dim3(256), 0, st, y, rcor.p, n);
            };
            eigs_smallest(st, n, op, EigsCsr{aptr.p, acol.p, aval.p}, (int)nev, (int)ncv, tol, max_restarts, tenv && tenv[0] == '1',
                          h->apps.Y.p, R);
        } catch (...) {
            restore();
            throw;
        }
        h->apps.last_solve[0] = h->apps.last_solve[1] = 0.0;
        if (C.cmg) {
            const PcgScal& sc = C.cmg->sc_host[0];
            h->apps.last_solve[0] = (double)sc.iter;
            h->apps.last_solve[1] = sc.bb > 0.0 ? std::sqrt(sc.rr / sc.bb) : 0.0;
        }
        restore();
        // correlations with the load on the host, in row order; unit norm; the sign rule:
        // corr >= 0, and where |corr| < 1e-12 the component of largest magnitude is positive
        std::vector<double>& Y = h->apps.Yh;
        Y = h->apps.Y.download();
        double fn = 0.0;
        for (double v : C.apps_f) fn += v * v;
        fn = std::sqrt(fn);
        for (int64_t k = 0; k < nev; ++k) {
            double* y = Y.data() + k * n;
            double yn = 0.0;
            for (int64_t i = 0; i < n; ++i) yn += y[i] * y[i];
            yn = std::sqrt(yn);
            if (yn > 0.0)
                for (int64_t i = 0; i < n; ++i) y[i] /= yn;
            double c = 0.0;
            int64_t big = 0;
            for (int64_t i = 0; i < n; ++i) {
                c += y[i] * C.apps_f[i];
                if (std::abs(y[i]) > std::abs(y[big])) big = i;
            }
            c = fn > 0.0 ? c / fn : 0.0;
            const bool flip = std::abs(c) >= 1.0e-12 ? c < 0.0 : y[big] < 0.0;
            if (flip) {
                for (int64_t i = 0; i < n; ++i) y[i] = -y[i];
                c = -c;
            }
            eigval[k] = R.theta[k];
            resid[k] = R.resid[k];
            corr[k] = c;
        }
        {
            SyncCallGuard g;
            DDPCA_HIP(hipMemcpy(h->apps.Y.p, Y.data(), Y.size() * sizeof(double), hipMemcpyHostToDevice));
        }
        h->apps.nev = (int)nev;
        std::memcpy(h->apps.ms, R.ms, sizeof(R.ms));
        if (info) {
            info[0] = R.steps;
            info[1] = R.restarts;
            info[2] = R.applies;
            info[3] = n;
        }
        if (!R.converged)
            throw ApiError(DDPCA_ENOCONV, "mcontact_gpu_apps: not converged after " + std::to_string(R.restarts) +
                                              " restarts (the best pairs are filled in)");
    });
}

// Mode k of the last mcontact_gpu_apps on the owned subdomain tv, OUTP_SUB1(accuProl[tv] y_k's
// rows of tv) (MCONTACT.h:2384-2393): the coarse correction's prolongation kernels into a zeroed
// scratch with the workspace's layout, the hanging level by the rows the ADMM step applies after
// a coarse correction
int64_t mcontact_gpu_apps_mode(mcontact_t h, int64_t k, int64_t tv, double* out, int64_t cap) {
    int64_t cnt = 0;
    const int rc = guarded([&] {
        if (!h) throw ApiError(DDPCA_EINVAL, "mcontact_gpu_apps_mode: NULL handle");
        if (h->apps.nev < 1) throw ApiError(DDPCA_ESTATE, "mcontact_gpu_apps_mode: no mcontact_gpu_apps result");
        if (k < 0 || k >= h->apps.nev) throw ApiError(DDPCA_EINVAL, "mcontact_gpu_apps_mode: mode index out of range");
        const ddpca_mcontact::Sub* S = nullptr;
        for (const auto& s : h->subs)
            if (s.tv == tv) S = &s;
        if (!S) throw ApiError(DDPCA_EINVAL, "subdomain not owned by this rank");
        cnt = 3 * S->nn + S->nh;
        if (!out) return;
        select_device(h->device);
        hipStream_t st = h->main;
        DevBuf<double> scratch((size_t)(h->NU + h->NH));
        scratch.zero(st);
        coarse_prolong(*h, h->apps.Y.p + (size_t)k * h->cs.n, scratch.p);
        if (h->NH) h->op_hang.apply(st, scratch.p, scratch.p + h->NU, nullptr);
        DDPCA_HIP(hipStreamSynchronize(st));
        SyncCallGuard g;
        DDPCA_HIP(hipMemcpy(out, scratch.p + S->dof0, std::min(3 * S->nn, cap) * sizeof(double), hipMemcpyDeviceToHost));
        if (cap > 3 * S->nn && S->nh)
            DDPCA_HIP(hipMemcpy(out + 3 * S->nn, scratch.p + h->NU + S->hoff, std::min(S->nh, cap - 3 * S->nn) * sizeof(double),
                                hipMemcpyDeviceToHost));
    });
    return rc < 0 ? rc : cnt;
}

int ddpca_eigs_orth_bench(int device, int64_t n, int m, int reps, double* out4) {
    return guarded([&] {
        if (!out4) throw ApiError(DDPCA_EINVAL, "ddpca_eigs_orth_bench: NULL output");
        eigs_orth_bench(device, n, m, reps, out4);
    });
}

int mcontact_gpu_destroy(mcontact_t h) {
    return guarded([&] {
        if (!h) return;
        (void)hipSetDevice(h->device);
        if (h->main) (void)hipStreamSynchronize(h->main);
        h->comm.reset();
        for (auto& e : h->ev)
            if (e) (void)hipEventDestroy(e);
        const bool own_stream = !h->mg && h->main;
        hipStream_t st = h->main;
        delete h;
        if (own_stream) (void)hipStreamDestroy(st);
    });
}

}  // extern "C"
