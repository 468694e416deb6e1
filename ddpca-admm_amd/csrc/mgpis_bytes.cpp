// Algorithmic byte model of the MGPIS solve path (mgpis_bytes.hpp).
#include "mgpis_bytes.hpp"

namespace ddpca {

double fine_matrix_bytes(const MgpisBytes& M, int s, int vt, bool prod_cols) {
    // operator bytes one fine-level pass reads for member s: streamed values = 4 B index + 72 B
    // (fp64), 36 B (fp32), 20 B (block-exponent fp16) or 10 B (block-scaled int8) per stored block; table mode = 4 B index per block +
    // 4 B row type per node + the member's share of the table (read once per launch)
    const MgpisBytes::Level& L = M.lev.back();
    // (the production kernels read 2-B column offsets where the level has them, prod_cols)
    const double cb = (prod_cols && L.col16) ? 2.0 : 4.0;
    if (!L.tbl) return (cb + vbytes(vt)) * (double)L.nnzb_sub[s];
    double nodes = 0.0;
    for (int64_t n : L.nloc) nodes += (double)n;
    return 4.0 * (double)L.nnzb_sub[s] + 4.0 * (double)L.nloc[s] +
           (double)L.ntypes * (double)L.tstride * 8.0 * (double)L.nloc[s] / nodes;
}

double fine_kernel_bytes(const MgpisBytes& M, int s) {
    // algorithmic bytes of one fine-level k_sell<kPcg> for member s: the operator + z gathered
    // once (24 B/node) + p, q read and written (4 x 24 B/node)
    return fine_matrix_bytes(M, s, kVal64) + 24.0 * 5.0 * (double)M.lev.back().nloc[s];
}

// ---- algorithmic byte model of the solve path (per member s; bytes every kernel must move at
// least once: streamed operator values + column indices, each vector read / written once, a
// gathered vector counted once per element).  The launch sequence is the one vcycle() and
// enqueue_iteration() issue; the sizes are the member's real (unpadded) nodes.

void vcycle_bytes(const MgpisBytes& M, int s, double out[2]) {
    out[0] = out[1] = 0.0;
    const auto& lev = M.lev;
    const MgpisBytes::Colours& gs = M.gs;
    const int nlev = (int)lev.size(), Lf = nlev - 1, cl = M.clev;
    const bool bj = M.smoother >= 1, cheb = M.smoother == 2;
    auto n = [&](int l) { return (double)lev[l].nloc[s]; };
    auto mat = [&](int l) {  // one pass over the V-cycle's copy of level l
        const MgpisBytes::Level& L = lev[l];
        if (L.tbl) return 4.0 * (double)L.nnzb_sub[s] + 4.0 * n(l);
        const double cb = L.col16 ? 2.0 : 4.0;
        return (vbytes(L.vt) + cb) * (double)L.nnzb_sub[s];
    };
    auto minv = [&](int l) { return (bj ? 9.0 : 3.0) * (lev[l].vt != kVal64 ? 4.0 : 8.0); };
    auto put = [&](int l, double b) { out[l == Lf ? 0 : 1] += b; };
    // x' = x + w M (b - K x): operator, x gathered, b, M^-1, x' (Chebyshev: d read + written); on a
    // level with fp32 iterate copies x is gathered in 16 B and x' written in 16 B, in fp64 by the
    // level's last sweep (fin)
    auto x4 = [&](int l) { return lev[l].x4; };
    auto sweep = [&](int l, bool fin = true) {
        if (x4(l)) return mat(l) + n(l) * (16.0 + 24.0 + (fin ? 24.0 : 16.0) + minv(l));
        return mat(l) + n(l) * (24.0 * 3 + minv(l) + (cheb ? 48.0 : 0.0));
    };
    const double n0 = 3.0 * (double)lev[cl].nloc[s];
    const double coarse = (M.ainv32 ? 4.0 : 8.0) * n0 * n0 + 16.0 * n0;  // dense inverse + b in, x out
    if (Lf == cl) {
        out[0] += coarse + 16.0 * n0;  // + the dot product's second read
        return;
    }
    const bool gsf = gs.ncol > 0;
    // multicolour sweeps on the fine level: L + U = the off-diagonal blocks, read once by the
    // forward sweep + residual pair and once by the backward sweep; per launch the x entries of
    // the colours it reads (forward colour k: the k earlier ones, residual: the later ones,
    // backward: all others), and per row b, M^-1, the row index and x (or r) written
    const double K = gsf ? (double)gs.ncol : 0.0;
    const double gsvb = gsf ? vbytes(gs.vt) + (gs.col16 ? 2.0 : 4.0) : 0.0;
    const double gsmat = gsvb * (gsf ? (double)gs.nnzb_sub[s] : 0.0);
    // rows the colours sweep (all of them unless band mode), and band mode's ring and far rows
    const double nsw = gsf && gs.band ? (double)gs.band_rows_sub[s] : n(Lf);
    const double nring = gsf && gs.band ? (double)gs.ring_rows_sub[s] : 0.0;
    const double nout = gsf && gs.band ? nring + (double)gs.far_rows_sub[s] : 0.0;
    // x4 mode (GsFine::x4): the iterate the sweeps gather and the forward sweep / prolongation
    // write is the 16-B fp32 copy; the backward sweep writes it and the fp64 output
    const double xb = gsf && gs.x4 ? 16.0 : 24.0;
    const double rb = gsf && gs.r4 ? 16.0 : 24.0;  // the residual written by the sweeps, read by the restriction
    const bool ssor = gsf && M.smoother == 4;
    if (ssor) {
        // colour SSOR: forward from zero (L; b, M^-1, x, w written), backward (U; b, w, M^-1 read, x
        // written), residual (L; w read, r written); x entries gathered as the Gauss-Seidel pair's
        const double lpass = gsmat * 0.5, upass = gsmat * 0.5, row = 4.0;
        put(Lf, lpass + nsw * (24.0 + minv(Lf) + xb + 24.0 + row + xb * (K - 1.0) / 2.0));
        put(Lf, upass + nsw * (48.0 + minv(Lf) + xb + row + xb * (K - 1.0) / 2.0));
        put(Lf, lpass + nsw * (24.0 + rb + row + xb * (K - 1.0) / 2.0));
    } else if (gsf) {
        put(Lf, 76.0 * nout);  // band mode: x = 0, r = b outside the colours (b read, x, r written, row index)
        put(Lf, gsmat + nsw * (24.0 + minv(Lf) + xb + 4.0 + xb * (K - 1.0) / 2.0));  // forward
        put(Lf, nsw * (rb + 4.0 + xb * (K - 1.0) / 2.0));                            // residual
        // band mode: the ring's residual over its band columns (blocks, b read, r written, x gathered)
        put(Lf, gsvb * (double)(gs.band ? gs.ring_nnzb_sub[s] : 0) + nring * (24.0 + 24.0 + 4.0 + 24.0));
    } else {
        put(Lf, n(Lf) * ((x4(Lf) ? 40.0 : 48.0) + minv(Lf) + (cheb ? 24.0 : 0.0)));  // k_jac0: b in, x out
    }
    for (int l = Lf; l >= cl + 1; --l) {
        if (!(gsf && l == Lf)) {
            for (int k = 1; k < M.nu; ++k) put(l, sweep(l, false));
            put(l, mat(l) + (x4(l) ? 64.0 : 72.0) * n(l));  // residual: x gathered, b, r
        }
        const MgpisBytes::Level& F = lev[l];
        const int c = l - 1;
        const bool init = c != cl;
        // coarse node: mask + b_c written (+ x_c = w M b_c: M^-1 read, x_c written; Chebyshev d_c)
        double cn = 1.0 + 24.0 + (init ? minv(c) + (x4(c) ? 16.0 : 24.0) + (cheb ? 24.0 : 0.0) : 0.0);
        double tr = (gsf && l == Lf ? rb : 24.0) * n(l);  // r_f read once
        if (F.lat) cn += 8.0;     // 27-bit child mask + fine copy
        else tr += 12.0 * (double)F.tent_sub[s];  // child index + weight per stencil entry
        tr += 4.0 * 8.0 * (double)F.tblk_sub[s] + (F.tblk_sub[s] ? 24.0 * n(c) : 0.0);  // block entries (B^T r_f)
        put(l, tr + cn * n(c));
    }
    put(cl, coarse);
    for (int l = cl + 1; l <= Lf; ++l) {
        const MgpisBytes::Level& F = lev[l];
        // x_f += mask P e_c: e_c read once, mask, x_f read + written, the parent encoding
        double pb = 24.0 * n(l - 1) + n(l) * (1.0 + (gsf && l == Lf ? 2.0 * xb : x4(l) ? 32.0 : 48.0));
        if (F.lat) pb += 4.0 * n(l);
        else pb += (F.uw ? 4.0 : 12.0) * (double)F.tent_sub[s];
        pb += 4.0 * 8.0 * (double)F.tblk_sub[s];
        put(l, pb);
        if (ssor && l == Lf) {
            // forward from the prolongated x (L + U; b, M^-1 read, x, w written), backward (U; b, w,
            // M^-1 read, z written)
            put(l, gsmat + nsw * (24.0 + minv(l) + xb + 24.0 + 4.0 + xb * (K - 1.0)));
            put(l, gsmat * 0.5 + nsw * (48.0 + minv(l) + 24.0 + 4.0 + xb * (K - 1.0) / 2.0));
            continue;
        }
        if (gsf && l == Lf) {
            put(l, gsmat + nsw * (24.0 + minv(l) + 24.0 + (xb < 24.0 ? xb : 0.0) + 4.0 + xb * (K - 1.0)));  // backward
            put(l, 52.0 * nout);  // band mode: b . x of the rows outside the colours (b, x read, row index)
            continue;
        }
        for (int k = 0; k < M.nu; ++k) put(l, sweep(l, k == M.nu - 1));
    }
}

void iteration_bytes(const MgpisBytes& M, int s, double out[2]) {
    vcycle_bytes(M, s, out);
    const MgpisBytes::Level& F = M.lev.back();
    const double n = (double)F.nloc[s], nch = (double)pad64(F.nloc[s]) / kChunk;
    out[0] += fine_kernel_bytes(M, s) + 144.0 * n;  // k_sell<kPcg> + k_axpy (x, r read + written, p, q read)
    out[1] += 3.0 * 8.0 * nch;                      // three k_fin passes over the chunk partials
}

void setup_bytes(const MgpisBytes& M, int s, double out[2]) {
    vcycle_bytes(M, s, out);
    const MgpisBytes::Level& F = M.lev.back();
    const double n = (double)F.nloc[s], nch = (double)pad64(F.nloc[s]) / kChunk;
    out[0] += 120.0 * n;  // k_pcg_init: b read, x r p q written
    out[1] += 2.0 * 8.0 * nch;
}

int64_t iteration_launches(const MgpisBytes& M) {
    // k_sell<kPcg>, k_axpy, 3 x k_fin, and the V-cycle: jac0 + per descended level (nu - 1 sweeps,
    // residual, restriction) + coarse + per ascended level (prolongation, nu sweeps); the
    // multicolour fine level: one forward and one backward launch per colour + the residual in
    // place of jac0, nu - 1 + 1 + nu sweep launches
    const bool gsf = M.gs.ncol > 0;
    const int64_t nd = (int64_t)M.lev.size() - 1 - M.clev;
    const int64_t base = 5 + (nd == 0 ? 2 : 1 + nd * (M.nu + 1) + 1 + nd * (1 + M.nu));
    // (band mode: + the x = 0 / r = b launch, the ring's residual and the dot of the other rows)
    if (gsf && nd > 0 && M.smoother == 4) return base - 1 - 2 * M.nu + 4 * M.gs.ncol + 1;  // colour SSOR
    return gsf && nd > 0 ? base - 1 - 2 * M.nu + 2 * M.gs.ncol + 1 + (M.gs.band ? 3 : 0) : base;
}

}  // namespace ddpca
