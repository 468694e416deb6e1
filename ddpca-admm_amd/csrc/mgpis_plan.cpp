// Host-side setup of MgpisDevice: see mgpis_plan.hpp.
#include "mgpis_plan.hpp"

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <numeric>
#include <string>
#include <unordered_map>

#include "common.hpp"

namespace ddpca {

MgpisTuning mgpis_tuning() {
    auto num = [](const char* name, int dflt) {
        const char* e = std::getenv(name);
        return e ? std::atoi(e) : dflt;
    };
    auto not0 = [](const char* name) {  // on unless the value starts with '0'
        const char* e = std::getenv(name);
        return !(e && e[0] == '0');
    };
    MgpisTuning t;
    t.col16 = num("DDPCA_COL16", 1) != 0;
    t.h16_levels = num("DDPCA_H16_LEVELS", 3);
    t.q8_levels = num("DDPCA_Q8_LEVELS", 64);
    t.gs_band = not0("DDPCA_GS_BAND");
    t.lattice = num("DDPCA_LATTICE", 1) != 0;
    t.gs_r32 = not0("DDPCA_GS_R32");
    t.bj_x4 = not0("DDPCA_BJ_X4");
    t.verbose = std::getenv("DDPCA_VERBOSE") != nullptr;
    return t;
}

// ============================================================================== small pieces
bool invert3(const double m[9], double r[9]) {
    const double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) +
                       m[2] * (m[3] * m[7] - m[4] * m[6]);
    if (!(std::abs(det) > 0.0)) return false;
    r[0] = (m[4] * m[8] - m[5] * m[7]) / det;
    r[1] = (m[2] * m[7] - m[1] * m[8]) / det;
    r[2] = (m[1] * m[5] - m[2] * m[4]) / det;
    r[3] = (m[5] * m[6] - m[3] * m[8]) / det;
    r[4] = (m[0] * m[8] - m[2] * m[6]) / det;
    r[5] = (m[2] * m[3] - m[0] * m[5]) / det;
    r[6] = (m[3] * m[7] - m[4] * m[6]) / det;
    r[7] = (m[1] * m[6] - m[0] * m[7]) / det;
    r[8] = (m[0] * m[4] - m[1] * m[3]) / det;
    return true;
}

void cheb_coef(double lmax, int k, double& c1, double& c2) {
    const double lmin = lmax / 30.0;
    const double theta = 0.5 * (lmax + lmin), delta = 0.5 * (lmax - lmin), sigma = theta / delta;
    if (k == 0) {
        c1 = 0.0;
        c2 = 1.0 / theta;
        return;
    }
    double rho_old = 1.0 / sigma, rho = rho_old;
    for (int i = 1; i <= k; ++i) {
        rho = 1.0 / (2.0 * sigma - rho_old);
        if (i < k) rho_old = rho;
    }
    c1 = rho * rho_old;
    c2 = 2.0 * rho / delta;
}

std::vector<double> smoother_coefs(const std::vector<double>& lmax, int nu, int smoother, double omega) {
    const int nsub = (int)lmax.size();
    std::vector<double> coef(2 * (nu + 1) * nsub, 0.0);
    for (int k = 0; k <= nu; ++k)
        for (int s = 0; s < nsub; ++s) {
            double c1 = 0.0, c2;
            if (smoother == 2) cheb_coef(lmax[s], k, c1, c2);
            else c2 = omega > 0.0 ? omega : (omega < 0.0 ? -omega : 4.0 / 3.0) / lmax[s];
            coef[2 * (k * nsub + s)] = c1;
            coef[2 * (k * nsub + s) + 1] = c2;
        }
    return coef;
}

std::vector<int32_t> free_dof_map(const SubdomainOps& S, const std::vector<int32_t>& p, int64_t noff) {
    std::vector<int32_t> f;
    for (int64_t d = 0; d < 3 * S.nnodes.back(); ++d)
        if (S.dof_free[d]) f.push_back((int32_t)(3 * (noff + p[d / 3]) + d % 3));
    return f;
}

// ============================================================================== numbering
namespace {
constexpr int64_t kMaxRowBlocks = 128;  // longest node-block row the table mode types (longer: streamed)

// Canonical slot order of row r: its blocks sorted by the neighbour's quantised offset from the
// row node -- independent of any numbering, so equal rows stay equal after renumbering.
void canonical_slots(const Bsr3& A, int64_t r, const std::vector<Key3>& key, int64_t* ord) {
    const int64_t len = A.ptr[r + 1] - A.ptr[r];
    for (int64_t t = 0; t < len; ++t) ord[t] = A.ptr[r] + t;
    const Key3& kr = key[r];
    std::sort(ord, ord + len, [&](int64_t u, int64_t v) {
        const Key3& a = key[A.col[u]];
        const Key3& b = key[A.col[v]];
        for (int d = 0; d < 3; ++d)
            if (a[d] - kr[d] != b[d] - kr[d]) return a[d] - kr[d] < b[d] - kr[d];
        return false;
    });
}
}  // namespace

std::vector<Key3> quantised_keys(const double* xyz, int64_t n) {
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    for (int64_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) {
            lo[a] = i ? std::min(lo[a], xyz[3 * i + a]) : xyz[3 * i + a];
            hi[a] = i ? std::max(hi[a], xyz[3 * i + a]) : xyz[3 * i + a];
        }
    const double ext = std::max({hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]});
    const double q = ext > 0.0 ? 1e-9 * ext : 1.0;
    std::vector<Key3> key(n);
    for (int64_t i = 0; i < n; ++i)
        key[i] = {std::llround((xyz[3 * i + 2] - lo[2]) / q), std::llround((xyz[3 * i + 1] - lo[1]) / q),
                  std::llround((xyz[3 * i] - lo[0]) / q)};
    return key;
}

std::vector<int32_t> device_order(const std::vector<Key3>& key, const std::vector<int32_t>* type) {
    const int64_t n = (int64_t)key.size();
    std::vector<int32_t> idx(n), p(n);
    std::iota(idx.begin(), idx.end(), 0);
    std::stable_sort(idx.begin(), idx.end(), [&](int32_t a, int32_t b) {
        if (type && (*type)[a] != (*type)[b]) return (*type)[a] < (*type)[b];
        return key[a] < key[b];
    });
    for (int64_t k = 0; k < n; ++k) p[idx[k]] = (int32_t)k;
    return p;
}

std::vector<int32_t> identity_order(int64_t n) {
    std::vector<int32_t> p(n);
    std::iota(p.begin(), p.end(), 0);
    return p;
}

std::vector<int32_t> row_types(const Bsr3& A, const uint8_t* fr, const std::vector<Key3>& key, int64_t& ntypes) {
    const int64_t n = A.nb;
    std::vector<int32_t> t(n);
    std::unordered_map<uint64_t, std::vector<int32_t>> bucket;
    std::vector<std::vector<double>> reps;
    std::vector<double> v;
    int64_t ord[kMaxRowBlocks];
    for (int64_t r = 0; r < n; ++r) {
        const int64_t len = A.ptr[r + 1] - A.ptr[r];
        canonical_slots(A, r, key, ord);
        v.assign(9 * len, 0.0);
        for (int64_t s = 0; s < len; ++s) {
            const int64_t k = ord[s], j = A.col[k];
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) {
                    double x = A.val[9 * k + 3 * a + b];
                    if (!fr[3 * r + a] || !fr[3 * j + b]) x = (j == r && a == b) ? 1.0 : 0.0;
                    v[9 * s + 3 * a + b] = x;
                }
        }
        uint64_t h = 1469598103934665603ull ^ (uint64_t)len;
        for (double x : v) {
            uint64_t b;
            std::memcpy(&b, &x, 8);
            h = (h ^ b) * 1099511628211ull;
            h ^= h >> 29;
        }
        auto& cand = bucket[h];
        int32_t id = -1;
        for (int32_t c : cand)
            if (reps[c].size() == v.size() && std::memcmp(reps[c].data(), v.data(), v.size() * sizeof(double)) == 0) {
                id = c;
                break;
            }
        if (id < 0) {
            id = (int32_t)reps.size();
            cand.push_back(id);
            reps.push_back(v);
        }
        t[r] = id;
    }
    ntypes = (int64_t)reps.size();
    return t;
}

MgpisNumbering mgpis_numbering(const std::vector<SubdomainOps>& subs, int table_mode) {
    const int nsub = (int)subs.size(), nlev = (int)subs[0].nnodes.size();
    MgpisNumbering N;
    N.perm.assign(nlev, std::vector<std::vector<int32_t>>(nsub));
    N.keys.assign(nlev, std::vector<std::vector<Key3>>(nsub));
    N.grouped.assign(nlev, 0);
    for (int l = 0; l < nlev; ++l) {
        bool geo = l > 0;
        for (int s = 0; s < nsub; ++s) geo = geo && subs[s].coords != nullptr;
        if (!geo) {
            for (int s = 0; s < nsub; ++s) N.perm[l][s] = identity_order(subs[s].nnodes[l]);
            continue;
        }
        std::vector<std::vector<int32_t>> types(nsub);
        double tab_blocks = 0.0, blocks = 0.0;
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : tab_blocks, blocks)
        for (int s = 0; s < nsub; ++s) {
            const Bsr3& A = *subs[s].K[l];
            N.keys[l][s] = quantised_keys(subs[s].coords, subs[s].nnodes[l]);
            if (table_mode == 0) continue;
            int64_t nt = 0, tmax = 0;
            for (int64_t r = 0; r < A.nb; ++r) tmax = std::max<int64_t>(tmax, A.ptr[r + 1] - A.ptr[r]);
            if (tmax > kMaxRowBlocks) continue;  // long rows: no table for this subdomain
            types[s] = row_types(A, subs[s].free_flags(l), N.keys[l][s], nt);
            tab_blocks += (double)nt * (double)tmax;
            blocks += (double)A.nnzb();
        }
        N.grouped[l] = table_mode == 2 || (table_mode == 1 && tab_blocks <= 0.2 * blocks);
        for (int s = 0; s < nsub; ++s)
            N.perm[l][s] = device_order(N.keys[l][s], N.grouped[l] && !types[s].empty() ? &types[s] : nullptr);
    }
    return N;
}

// ============================================================================== level plan
namespace {
// Table mode of one level: every row's values (device slot order, masks applied, zero beyond the
// row) are deduplicated bit-exactly, per subdomain in parallel, then merged into one table.  Used
// when the table is at most a fifth of the streamed values (or when forced, for tests).
void plan_table(LevelPlan& L, bool force) {
    const auto &slots = L.slots;
    const auto &off = L.off;
    const auto &val = L.val;
    int64_t tmax = 0;
    for (int32_t s : slots) tmax = std::max<int64_t>(tmax, s);
    const int64_t ts9 = std::max<int64_t>(tmax * 9, 1);
    const int nsub = (int)L.noff.size();
    std::vector<std::vector<double>> subtab(nsub);
    std::vector<int32_t> rt(L.nn, 0);
#pragma omp parallel for schedule(dynamic, 1)
    for (int s = 0; s < nsub; ++s) {
        std::unordered_map<uint64_t, std::vector<int32_t>> bucket;
        std::vector<double>& T = subtab[s];
        std::vector<double> rowv(ts9);
        int32_t nt = 0;
        for (int64_t g = L.noff[s]; g < L.noff[s] + pad64(L.nloc[s]); ++g) {
            const int64_t c = g / kChunk, lane = g % kChunk;
            std::fill(rowv.begin(), rowv.end(), 0.0);
            for (int64_t t = 0; t < slots[c]; ++t)
                for (int ij = 0; ij < 9; ++ij) rowv[t * 9 + ij] = val[((off[c] + t) * 9 + ij) * kChunk + lane];
            uint64_t h = 1469598103934665603ull;
            for (double v : rowv) {
                uint64_t b;
                std::memcpy(&b, &v, 8);
                h = (h ^ b) * 1099511628211ull;
                h ^= h >> 29;
            }
            int32_t id = -1;
            auto& cand = bucket[h];
            for (int32_t t : cand)
                if (std::memcmp(&T[(size_t)t * ts9], rowv.data(), ts9 * sizeof(double)) == 0) {
                    id = t;
                    break;
                }
            if (id < 0) {
                id = nt++;
                cand.push_back(id);
                T.insert(T.end(), rowv.begin(), rowv.end());
            }
            rt[g] = id;
        }
    }
    int64_t ntypes = 0;
    std::vector<int64_t> base(nsub);
    for (int s = 0; s < nsub; ++s) {
        base[s] = ntypes;
        ntypes += (int64_t)subtab[s].size() / ts9;
    }
    const double tab_bytes = (double)ntypes * ts9 * 8.0, val_bytes = (double)val.size() * 8.0;
    if (!force && tab_bytes > 0.2 * val_bytes) return;
    L.tab.reserve((size_t)ntypes * ts9);
    for (int s = 0; s < nsub; ++s) {
        L.tab.insert(L.tab.end(), subtab[s].begin(), subtab[s].end());
        for (int64_t g = L.noff[s]; g < L.noff[s] + pad64(L.nloc[s]); ++g) rt[g] += (int32_t)base[s];
    }
    // chunks whose 64 rows share one type read their table row through scalar loads
    L.ctype.resize(L.nch);
    int64_t uniform = 0;
    for (int64_t c = 0; c < L.nch; ++c) {
        int32_t& ct = L.ctype[c];
        ct = rt[c * kChunk];
        for (int64_t lane = 1; lane < kChunk && ct >= 0; ++lane)
            if (rt[c * kChunk + lane] != ct) ct = -1;
        uniform += ct >= 0;
    }
    L.tbl = true;
    L.tstride = ts9;
    L.ntypes = ntypes;
    L.nuniform = uniform;
    L.rtype = std::move(rt);
}
}  // namespace

LevelPlan plan_level(const std::vector<SubdomainOps>& subs, const MgpisNumbering& num, int l, bool bj, int table_mode,
                     const MgpisTuning& tune) {
    const int nsub = (int)subs.size();
    LevelPlan L;
    L.noff.resize(nsub);
    L.nloc.resize(nsub);
    int64_t tot = 0;
    for (int s = 0; s < nsub; ++s) {
        L.noff[s] = tot;
        L.nloc[s] = subs[s].nnodes[l];
        tot += pad64(L.nloc[s]);
    }
    L.nn = tot;
    L.nch = tot / kChunk;
    auto &slots = L.slots, &csub = L.csub, &col = L.col;
    auto &off = L.off;
    auto &val = L.val, &dinv = L.dinv, &minv = L.minv;
    auto &mask = L.mask;
    slots.assign(L.nch, 0);
    csub.assign(L.nch, 0);
    off.assign(L.nch + 1, 0);
    for (int s = 0; s < nsub; ++s) {
        const Bsr3& A = *subs[s].K[l];
        const auto& p = num.perm[l][s];
        const int64_t c0 = L.noff[s] / kChunk;
        for (int64_t c = c0; c < c0 + pad64(L.nloc[s]) / kChunk; ++c) csub[c] = s;
        for (int64_t r = 0; r < L.nloc[s]; ++r) {
            int32_t& sl = slots[c0 + p[r] / kChunk];
            sl = std::max<int32_t>(sl, (int32_t)(A.ptr[r + 1] - A.ptr[r]));
        }
        L.nnzb += A.nnzb();
        L.nnzb_sub.push_back(A.nnzb());
    }
    for (int64_t c = 0; c < L.nch; ++c) off[c + 1] = off[c] + slots[c];
    L.nslots = off[L.nch];
    col.assign(L.nslots * kChunk, 0);
    val.assign(L.nslots * kChunk * 9, 0.0);
    dinv.assign(3 * L.nn, 0.0);
    minv.assign(bj ? 9 * L.nn : 3 * L.nn, 0.0);
    mask.assign(L.nn, 0);
    for (int s = 0; s < nsub; ++s) {
        const Bsr3& A = *subs[s].K[l];
        const uint8_t* fr = subs[s].free_flags(l);  // reference order: level-l nodes are a prefix
        const auto& p = num.perm[l][s];
        const auto& keys = num.keys[l][s];
        const int64_t base = L.noff[s];
        // padded rows of the subdomain: self column, zero values
        for (int64_t r = L.nloc[s]; r < pad64(L.nloc[s]); ++r) {
            const int64_t g = base + r, c = g / kChunk, lane = g % kChunk;
            for (int64_t q = off[c]; q < off[c + 1]; ++q) col[q * kChunk + lane] = (int32_t)g;
        }
#pragma omp parallel for schedule(static)
        for (int64_t r = 0; r < L.nloc[s]; ++r) {
            const int64_t g = base + p[r], c = g / kChunk, lane = g % kChunk;
            uint8_t m = 0;
            for (int a = 0; a < 3; ++a) m |= fr[3 * r + a] ? (1 << a) : 0;
            mask[g] = m;
            // this row's blocks in canonical order (= increasing device column under the
            // lexicographic numbering), else in increasing device column
            const int64_t len = A.ptr[r + 1] - A.ptr[r];
            thread_local std::vector<int64_t> ordv;  // rows of any length (LAGRANGE's condensed systems)
            ordv.resize(len);
            int64_t* ord = ordv.data();
            if (!keys.empty()) {
                canonical_slots(A, r, keys, ord);
            } else {
                for (int64_t t = 0; t < len; ++t) ord[t] = A.ptr[r] + t;
                std::sort(ord, ord + len, [&](int64_t u, int64_t v) { return p[A.col[u]] < p[A.col[v]]; });
            }
            double diag[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (int64_t t = 0; t < len; ++t) {
                const int64_t k = ord[t], q = off[c] + t;
                const int64_t j = A.col[k];
                col[q * kChunk + lane] = (int32_t)(base + p[j]);
                for (int a = 0; a < 3; ++a)
                    for (int b = 0; b < 3; ++b) {
                        double v = A.val[9 * k + 3 * a + b];
                        if (!fr[3 * r + a] || !fr[3 * j + b]) v = (j == r && a == b) ? 1.0 : 0.0;
                        val[(q * 9 + 3 * a + b) * kChunk + lane] = v;
                        if (j == r) diag[3 * a + b] = v;
                    }
            }
            for (int64_t q = off[c] + len; q < off[c + 1]; ++q) col[q * kChunk + lane] = (int32_t)g;
            for (int a = 0; a < 3; ++a) dinv[3 * g + a] = fr[3 * r + a] ? 1.0 / diag[4 * a] : 0.0;
            if (bj) {
                double inv[9];
                if (!invert3(diag, inv)) for (int q = 0; q < 9; ++q) inv[q] = 0.0;
                for (int a = 0; a < 3; ++a)
                    for (int b = 0; b < 3; ++b)
                        minv[9 * g + 3 * a + b] = (fr[3 * r + a] && fr[3 * r + b]) ? inv[3 * a + b] : 0.0;
            } else {
                for (int a = 0; a < 3; ++a) minv[3 * g + a] = dinv[3 * g + a];
            }
        }
    }
    if (tune.col16) {
        // relative 16-bit columns when every offset of the level fits
        bool fits = true;
        std::vector<int16_t> col16(col.size());
        for (int64_t c = 0; c < L.nch && fits; ++c)
            for (int64_t q = off[c]; q < off[c + 1] && fits; ++q)
                for (int64_t lane = 0; lane < kChunk; ++lane) {
                    const int64_t d = (int64_t)col[q * kChunk + lane] - (c * kChunk + lane);
                    if (d < INT16_MIN || d > INT16_MAX) { fits = false; break; }
                    col16[q * kChunk + lane] = (int16_t)d;
                }
        if (fits) L.col16 = std::move(col16);
        L.fits16 = fits;
    }
    if (table_mode != 0 && l >= 1) plan_table(L, table_mode == 2 || num.grouped[l]);
    if (tune.verbose)
        std::fprintf(stderr, "[ddpca] level %d: %lld nodes, %lld chunks, %lld slots, table %d (%lld types, %lld uniform chunks)\n",
                     l, (long long)L.nn, (long long)L.nch, (long long)L.nslots, (int)L.tbl, (long long)L.ntypes,
                     (long long)L.nuniform);
    return L;
}

std::vector<float> smoother_inverse_fp32(const std::vector<double>& minv, bool bj, bool symmetrise) {
    std::vector<float> m32(minv.size());
    const int w = bj ? 9 : 3;
    const int64_t nn = (int64_t)minv.size() / w;
#pragma omp parallel for schedule(static)
    for (int64_t g = 0; g < nn; ++g) {
        const double* m = minv.data() + w * g;
        for (int k = 0; k < w; ++k)
            m32[w * g + k] = bj && symmetrise ? (float)(0.5 * (m[k] + m[3 * (k % 3) + k / 3])) : (float)m[k];
    }
    return m32;
}

// ============================================================================== value records
BlockValues::BlockValues(int vt_, int64_t nslot, bool sparse) : vt(vt_) {
    n = (size_t)nslot * vals_per_block(vt) * kChunk;
    if (sparse) n = std::max<size_t>(n, 1);
    if (vt == kValQ8) v8.assign(n, 0);
    else if (vt == kValH16) v16.assign(n, 0);  // zero blocks: e = 0, values 0
    else if (vt == kVal32) v32.assign(n, 0.0f);
    else v64.reset(sparse ? new double[n]() : new double[n]);
}

void BlockValues::put(int64_t slot, int64_t lane, const double* src, int64_t stride) {
    double blk[9];
    for (int ij = 0; ij < 9; ++ij) blk[ij] = src[ij * stride];
    if (vt == kValH16) {
        uint16_t rec[10];
        to_h16_block(blk, rec);
        for (int k = 0; k < 10; ++k) v16[slot * 10 * kChunk + h16_pos(k, lane)] = rec[k];
    } else if (vt == kValQ8) {
        uint8_t rec[12];
        if (!to_q8_block(blk, rec)) __atomic_store_n(&ok, false, __ATOMIC_RELAXED);  // (put runs in omp loops)
        for (int k = 0; k < 12; ++k) v8[slot * 12 * kChunk + q8_pos(k, lane)] = rec[k];
    } else if (vt == kVal32) {
        for (int ij = 0; ij < 9; ++ij) v32[slot * 9 * kChunk + slot_elem<float>(ij, lane)] = (float)blk[ij];
    } else {
        for (int ij = 0; ij < 9; ++ij) v64[slot * 9 * kChunk + slot_elem<double>(ij, lane)] = blk[ij];
    }
}

BlockValues pack_values(const LevelPlan& P, int vt) {
    BlockValues V(vt, P.nslots, false);
    const int64_t nslot = P.nslots;
#pragma omp parallel for schedule(static)
    for (int64_t q = 0; q < nslot; ++q)
        for (int64_t lane = 0; lane < kChunk; ++lane) V.put(q, lane, &P.val[q * 9 * kChunk + lane], kChunk);
    return V;
}

int level_copy_type(int precond_fp32, int l, int nlev, const MgpisTuning& tune) {
    if (!(l >= nlev - tune.h16_levels && precond_fp32 >= 2)) return kVal32;
    return precond_fp32 >= 3 && l >= nlev - tune.q8_levels ? kValQ8 : kValH16;
}

BlockValues level_copy(const LevelPlan& P, int vt, int l, const MgpisTuning& tune) {
    BlockValues V = pack_values(P, vt);
    if (V.ok) return V;
    if (tune.verbose) std::fprintf(stderr, "[ddpca] level %d: int8 scale out of range, block-exponent fp16 copy instead\n", l);
    return pack_values(P, kValH16);
}

// ============================================================================== transfers
namespace {
using KidList = std::vector<std::vector<std::pair<int32_t, double>>>;

bool lattice_reject(bool verbose, int why) {
    if (verbose) std::fprintf(stderr, "[ddpca] lattice transfer rejected (check %d)\n", why);
    return false;
}

// Lattice form of a uniformly averaging transfer l-1 -> l (TransferPlan::lat): accepted only when it
// reproduces the explicit lists exactly, per subdomain: every fine node's parent set is p0 plus
// the subset sums of three coarse strides (the differences of the two-parent nodes), every coarse
// node's child set is its fine copy plus d . t for d in {-1,0,1}^3 (t from the half-weight
// children) with weight 2^-|d|, the 27 offsets distinct.  Box lattices numbered lexicographically
// (the device renumbering of levels >= 1) pass; anything else keeps the explicit lists.
bool lattice_transfer(TransferPlan& T, const LevelShape& L, const LevelShape& C, const KidList& kids, bool verbose) {
    auto reject = [verbose](int why) { return lattice_reject(verbose, why); };
    const std::vector<int32_t>& ppar = T.ppar;
    const size_t ns = L.noff.size();
    std::vector<uint32_t> ppk(L.nn, 0u), rmsk(C.nn, 0u);
    std::vector<int32_t> pstr(3 * ns, 0), rstr(3 * ns, 0), rf0(C.nn, 0);
    if (C.nn >= (int64_t)1 << 29 || L.nn >= (int64_t)1 << 31) return reject(0);
    auto three = [&](std::vector<int64_t>& d, int32_t* out, int64_t fill) {
        std::sort(d.begin(), d.end());
        d.erase(std::unique(d.begin(), d.end()), d.end());
        if (d.size() > 3 || (!d.empty() && d[0] <= 0)) return reject(1);
        for (int k = 0; k < 3; ++k) out[k] = (int32_t)(k < (int)d.size() ? d[k] : fill + k);
        return true;
    };
    for (size_t s = 0; s < ns; ++s) {
        // prolongation
        std::vector<int64_t> d;
        int32_t P[8];
        auto parents = [&](int64_t gf) {
            int np = 0;
            while (np < 8 && ppar[np * L.nn + gf] >= 0) {
                P[np] = ppar[np * L.nn + gf];
                ++np;
            }
            std::sort(P, P + np);
            return np;
        };
        const int64_t f_lo = L.noff[s], f_hi = f_lo + L.nloc[s];
        for (int64_t gf = f_lo; gf < f_hi; ++gf)
            if (parents(gf) == 2) d.push_back((int64_t)P[1] - P[0]);
        int32_t* st = &pstr[3 * s];
        if (!three(d, st, (int64_t)1 << 28)) return reject(2);
        for (int64_t gf = f_lo; gf < f_hi; ++gf) {
            const int np = parents(gf);
            if (np != 1 && np != 2 && np != 4 && np != 8) return reject(3);
            bool found = false;
            for (uint32_t code = 0; code < 8 && !found; ++code) {
                if ((1 << __builtin_popcount(code)) != np) continue;
                int64_t set[8];
                int m = 0;
                for (uint32_t q = 0; q < 8; ++q)
                    if ((q & ~code) == 0)
                        set[m++] = P[0] + ((q & 1) ? st[0] : 0) + ((q & 2) ? st[1] : 0) + ((q & 4) ? (int64_t)st[2] : 0);
                std::sort(set, set + m);
                bool eq = true;
                for (int k = 0; k < m; ++k) eq &= set[k] == P[k];
                if (eq) {
                    ppk[gf] = (uint32_t)P[0] | (code << 29);
                    found = true;
                }
            }
            if (!found) return reject(4);
        }
        // restriction
        const int64_t c_lo = C.noff[s], c_hi = c_lo + C.nloc[s];
        d.clear();
        for (int64_t j = c_lo; j < c_hi; ++j) {
            if (kids[j].empty() || kids[j][0].second != 1.0) return reject(5);
            for (const auto& k : kids[j])
                if (k.second == 0.5) d.push_back(std::abs((int64_t)k.first - kids[j][0].first));
        }
        int32_t* t = &rstr[3 * s];
        if (!three(d, t, (int64_t)1 << 29)) return reject(6);
        std::vector<std::pair<int64_t, int>> offs;  // offset -> bit
        for (int q = 0; q < 27; ++q)
            offs.push_back({(int64_t)(q % 3 - 1) * t[0] + (int64_t)((q / 3) % 3 - 1) * t[1] + (int64_t)(q / 9 - 1) * t[2], q});
        std::sort(offs.begin(), offs.end());
        for (int q = 1; q < 27; ++q)
            if (offs[q].first == offs[q - 1].first) return reject(7);
        for (int64_t j = c_lo; j < c_hi; ++j) {
            const int64_t f0 = kids[j][0].first;
            uint32_t msk = 0;
            for (const auto& k : kids[j]) {
                const int64_t o = (int64_t)k.first - f0;
                auto it = std::lower_bound(offs.begin(), offs.end(), std::make_pair(o, -1));
                if (it == offs.end() || it->first != o) return reject(8);
                const int q = it->second;
                const int nz = (q % 3 != 1) + ((q / 3) % 3 != 1) + (q / 9 != 1);
                if (k.second != 1.0 / (double)(1 << nz) || ((msk >> q) & 1u)) return reject(9);
                msk |= 1u << q;
            }
            rmsk[j] = msk;
            rf0[j] = (int32_t)f0;
        }
    }
    T.lat = true;
    T.uw = true;
    T.ppk = std::move(ppk);
    T.pstr = std::move(pstr);
    T.rmsk = std::move(rmsk);
    T.rf0 = std::move(rf0);
    T.rstr = std::move(rstr);
    return true;
}
}  // namespace

TransferPlan plan_transfer(const std::vector<SubdomainOps>& subs, const MgpisNumbering& num, int l, const LevelShape& L,
                           const LevelShape& C, const MgpisTuning& tune) {
    const int nsub = (int)subs.size();
    TransferPlan T;
    auto &ppar = T.ppar;
    auto &pw = T.pw;
    ppar.assign(8 * L.nn, -1);
    pw.assign(8 * L.nn, 0.0);
    bool uw = true;  // every weight == 1 / the node's parent count
    KidList kids(C.nn);
    struct ExtraEnt {
        int32_t f, c;
        double b[9];
    };
    std::deque<ExtraEnt> extra;  // scalar parents past the eighth, as blocks
    T.tent_sub.assign(nsub, 0);
    T.tblk_sub.assign(nsub, 0);
    for (int s = 0; s < nsub; ++s) {
        const Stencil& st = *subs[s].S[l - 1];
        const auto& pf = num.perm[l][s];
        const auto& pc = num.perm[l - 1][s];
        const int64_t nc = C.nloc[s];
        if (st.nf != L.nloc[s] || st.nc != nc) throw ApiError(DDPCA_EINVAL, "stencil shape");
        T.tblk_sub[s] = (int64_t)st.bent.size();
        T.tent_sub[s] = (int64_t)st.col.size() - T.tblk_sub[s];
        // block entries (weight 0 in the scalar stencil) run in k_prolong_rot / k_restrict_rot
        // only: they take no parent slot (a node may have any number of them)
        std::vector<uint8_t> isblk(st.col.size(), 0);
        for (int64_t e : st.bent) isblk[e] = 1;
        if (!st.bent.empty()) uw = false;
        for (int64_t i = 0; i < L.nloc[s]; ++i) {
            int64_t np = 0;
            for (int64_t e = st.ptr[i]; e < st.ptr[i + 1]; ++e) np += !isblk[e];
            const int64_t gf = L.noff[s] + pf[i];
            if (i < nc) {
                if (np != 1 || st.col[st.ptr[i]] != i || st.w[st.ptr[i]] != 1.0)
                    throw ApiError(DDPCA_EINVAL, "stencil is not identity on coarse nodes");
                const int64_t gc = C.noff[s] + pc[i];
                ppar[gf] = (int32_t)gc;
                pw[gf] = 1.0;
                kids[gc].insert(kids[gc].begin(), {(int32_t)gf, 1.0});
                continue;
            }
            // parents past the eighth (LAGRANGE's condensed transfers) run as w*I blocks
            if (np > 8) uw = false;
            int64_t k = 0;
            for (int64_t e = st.ptr[i]; e < st.ptr[i + 1]; ++e) {
                if (isblk[e]) continue;
                if (k == 8) {
                    extra.push_back({(int32_t)gf, (int32_t)(C.noff[s] + pc[st.col[e]]), {}});
                    for (int q = 0; q < 9; ++q) extra.back().b[q] = q % 4 == 0 ? st.w[e] : 0.0;
                    continue;
                }
                if (st.w[e] != 1.0 / (double)np) uw = false;
                const int64_t gc = C.noff[s] + pc[st.col[e]];
                ppar[k * L.nn + gf] = (int32_t)gc;
                pw[k * L.nn + gf] = st.w[e];
                kids[gc].push_back({(int32_t)gf, st.w[e]});
                ++k;
            }
        }
    }
    // restriction children in SELL-64 over the coarse chunks; padding slots carry weight 0
    // on the node's own first child (or fine node 0 for padding nodes)
    auto &rsl = T.rslots, &rcol = T.rcol;
    auto &rof = T.roff;
    auto &rwt = T.rwt;
    rsl.assign(C.nch, 0);
    rof.assign(C.nch + 1, 0);
    for (int64_t c = 0; c < C.nch; ++c) {
        size_t mx = 0;
        for (int64_t j = c * kChunk; j < (c + 1) * kChunk; ++j) mx = std::max(mx, kids[j].size());
        rsl[c] = (int32_t)mx;
        rof[c + 1] = rof[c] + (int64_t)mx;
    }
    rcol.assign(std::max<int64_t>(rof[C.nch] * kChunk, 1), 0);
    rwt.assign(std::max<int64_t>(rof[C.nch] * kChunk, 1), 0.0);
    for (int64_t j = 0; j < C.nn; ++j) {
        const int64_t c = j / kChunk, lane = j % kChunk;
        for (int64_t k = 0; k < rsl[c]; ++k) {
            const int64_t q = (rof[c] + k) * kChunk + lane;
            const bool real = k < (int64_t)kids[j].size();
            rcol[q] = real ? kids[j][k].first : (kids[j].empty() ? 0 : kids[j][0].first);
            rwt[q] = real ? kids[j][k].second : 0.0;
        }
    }
    // block entries: (fine node, coarse node, 3x3) in batch-global indices, as CSR by
    // fine node (prolongation) and by coarse node (restriction)
    struct RotEnt {
        int32_t f, c;
        const double* b;
    };
    std::vector<RotEnt> ents;
    for (int s = 0; s < nsub; ++s) {
        const Stencil& st = *subs[s].S[l - 1];
        if (st.bent.empty()) continue;
        const auto& pf = num.perm[l][s];
        const auto& pc = num.perm[l - 1][s];
        int64_t i = 0;
        for (size_t q = 0; q < st.bent.size(); ++q) {
            const int64_t e = st.bent[q];
            while (st.ptr[i + 1] <= e) ++i;
            if (st.w[e] != 0.0) throw ApiError(DDPCA_EINVAL, "block transfer entry with a scalar weight");
            ents.push_back({(int32_t)(L.noff[s] + pf[i]), (int32_t)(C.noff[s] + pc[st.col[e]]), &st.bval[9 * q]});
        }
    }
    for (const ExtraEnt& x : extra) ents.push_back({x.f, x.c, x.b});
    if (!ents.empty()) {
        auto csr = [&](bool by_fine, int64_t& nr, std::vector<int32_t>& r, std::vector<int64_t>& pt, std::vector<int32_t>& o,
                       std::vector<double>& bv) {
            std::stable_sort(ents.begin(), ents.end(), [by_fine](const RotEnt& a, const RotEnt& b) {
                return by_fine ? a.f < b.f : a.c < b.c;
            });
            pt.assign(1, 0);
            for (size_t q = 0; q < ents.size(); ++q) {
                const int32_t key = by_fine ? ents[q].f : ents[q].c;
                if (r.empty() || r.back() != key) {
                    if (!r.empty()) pt.push_back((int64_t)q);
                    r.push_back(key);
                }
                o.push_back(by_fine ? ents[q].c : ents[q].f);
                bv.insert(bv.end(), ents[q].b, ents[q].b + 9);
            }
            pt.push_back((int64_t)ents.size());
            nr = (int64_t)r.size();
        };
        csr(true, T.nrot, T.rot_row, T.rot_ptr, T.rot_par, T.rot_blk);
        csr(false, T.nrotc, T.rotc_row, T.rotc_ptr, T.rotc_kid, T.rotc_blk);
    }
    if (tune.lattice && uw && ents.empty() && lattice_transfer(T, L, C, kids, tune.verbose)) {
        if (tune.verbose) std::fprintf(stderr, "[ddpca] level %d: lattice transfers\n", l);
        return T;
    }
    if (tune.verbose)
        std::fprintf(stderr, "[ddpca] level %d: explicit transfer lists (uniform averaging %d, block entries %zu)\n", l,
                     (int)uw, ents.size());
    T.uw = uw;  // prolongation weights from the parent count (restriction keeps rwt)
    return T;
}

// ============================================================================== colours
std::vector<uint8_t> colour_band(const std::vector<SubdomainOps>& subs, const MgpisNumbering& num, int l, const LevelPlan& L,
                                 const MgpisTuning& tune) {
    if (!tune.gs_band) return {};
    std::vector<uint8_t> bandv(L.nn, 0);
    int64_t nreal = 0, nband = 0;
    for (size_t s = 0; s < subs.size(); ++s) {
        nreal += L.nloc[s];
        for (int64_t ref = subs[s].nnodes[l - 1]; ref < subs[s].nnodes[l]; ++ref)
            bandv[L.noff[s] + num.perm[l][s][ref]] = 2;  // new node
    }
    for (int64_t g = 0; g < L.nn; ++g) {
        if (bandv[g] != 2) continue;
        const int64_t c = g / kChunk, lane = g % kChunk;
        for (int64_t q = L.off[c]; q < L.off[c + 1]; ++q) {
            bool nz = false;
            for (int ij = 0; ij < 9 && !nz; ++ij) nz = L.val[(q * 9 + ij) * kChunk + lane] != 0.0;
            const int64_t j = L.col[q * kChunk + lane];
            if (nz && bandv[j] == 0) bandv[j] = 1;
        }
    }
    for (uint8_t f : bandv) nband += f != 0;
    if (nband == 0 || nband > (nreal * 3) / 5) bandv.clear();
    return bandv;
}

// A colour's rows go to chunks in device order, i.e. along the x lines of a box (16 x 16-node
// tiles of one plane measured 1.8 % slower at the headline, profiles/r03i).
ColourPlan plan_colours(const LevelPlan& L, int vt, const std::vector<float>* minv32, const std::vector<uint8_t>* band,
                        const MgpisTuning& tune) {
    const int nsub = (int)L.noff.size();
    const auto &off = L.off;
    const auto &col = L.col;
    const auto &val = L.val;
    ColourPlan G;
    // greedy colouring in device order, per member
    std::vector<int8_t> colour(L.nn, -1);
    std::vector<int> ncol_sub(nsub, 0);
    int too_many = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(max : too_many)
    for (int s = 0; s < nsub; ++s) {
        for (int64_t g = L.noff[s]; g < L.noff[s] + L.nloc[s]; ++g) {
            if (band && !(*band)[g]) continue;
            const int64_t c = g / kChunk, lane = g % kChunk;
            uint64_t used = 0;
            for (int64_t q = off[c]; q < off[c + 1]; ++q) {
                const int64_t j = col[q * kChunk + lane];
                if (j != g && colour[j] >= 0) used |= 1ull << colour[j];
            }
            if (used == ~0ull) {
                too_many = 1;
                break;
            }
            const int k = __builtin_ctzll(~used);
            colour[g] = (int8_t)k;
            ncol_sub[s] = std::max(ncol_sub[s], k + 1);
        }
    }
    if (too_many) throw ApiError(DDPCA_EINVAL, "multicolour smoother: a node graph needing more than 64 colours");
    const int K = *std::max_element(ncol_sub.begin(), ncol_sub.end());
    // chunk groups per member: the colours, then (band mode) the ring and the far rows
    const int KG = band ? K + 2 : K;
    auto is_band = [&](int64_t j) { return colour[j] >= 0; };
    // colour chunks, member-major and colour-minor
    std::vector<std::vector<int64_t>> rows((size_t)nsub * KG);
    for (int s = 0; s < nsub; ++s)
        for (int64_t g = L.noff[s]; g < L.noff[s] + L.nloc[s]; ++g) {
            int grp = colour[g];
            if (grp < 0) {
                grp = K + 1;  // far unless a neighbour is in the band
                const int64_t nc = g / kChunk, lane = g % kChunk;
                for (int64_t q = off[nc]; q < off[nc + 1] && grp == K + 1; ++q) {
                    const int64_t j = col[q * kChunk + lane];
                    if (j != g && is_band(j)) grp = K;
                }
            }
            rows[(size_t)s * KG + grp].push_back(g);
        }
    // which neighbours a row of group k stores: colours L = earlier colours and every non-band
    // column (x = 0 there in the forward sweep), U = the rest; ring rows: their band columns as L
    auto store = [&](int k, int64_t j) -> int {  // 0 L, 1 U, -1 not stored
        if (k < K) return colour[j] < k ? 0 : 1;
        if (k == K) return is_band(j) ? 0 : -1;
        return -1;
    };
    auto &rowidx = G.rowidx, &csub = G.csub, &nsl = G.nsl, &nsu = G.nsu;
    auto &offl = G.offl, &offu = G.offu, &cb = G.cb;
    cb.assign(nsub + 1, 0);
    std::vector<std::vector<int32_t>> bycol(KG);
    std::vector<int64_t> base;  // first row of each chunk in its (s, k) list
    std::vector<size_t> lists;
    G.nnzb_sub.assign(nsub, 0);
    G.slots_sub.assign(nsub, 0);
    G.band = band != nullptr;
    G.band_rows_sub.assign(nsub, 0);
    G.ring_rows_sub.assign(nsub, 0);
    G.far_rows_sub.assign(nsub, 0);
    G.ring_nnzb_sub.assign(nsub, 0);
    for (int s = 0; s < nsub; ++s) {
        cb[s] = (int64_t)csub.size();
        for (int k = 0; k < KG; ++k) {
            const auto& R = rows[(size_t)s * KG + k];
            (k < K ? G.band_rows_sub : k == K ? G.ring_rows_sub : G.far_rows_sub)[s] += (int64_t)R.size();
            for (size_t r0 = 0; r0 < R.size(); r0 += kChunk) {
                const int64_t c = (int64_t)csub.size();
                bycol[k].push_back((int32_t)c);
                csub.push_back(s);
                base.push_back((int64_t)r0);
                lists.push_back((size_t)s * KG + k);
                int32_t ml = 0, mu = 0;
                for (size_t i = r0; i < std::min(R.size(), r0 + kChunk); ++i) {
                    const int64_t g = R[i], nc = g / kChunk, lane = g % kChunk;
                    int32_t nl = 0, nu = 0;
                    for (int64_t q = off[nc]; q < off[nc + 1]; ++q) {
                        const int64_t j = col[q * kChunk + lane];
                        if (j == g) continue;
                        const int t = store(k, j);
                        if (t == 0) ++nl;
                        else if (t == 1) ++nu;
                    }
                    ml = std::max(ml, nl);
                    mu = std::max(mu, nu);
                    (k < K ? G.nnzb_sub : G.ring_nnzb_sub)[s] += nl + nu;
                }
                nsl.push_back(ml);
                nsu.push_back(mu);
            }
        }
    }
    const int64_t nch = (int64_t)csub.size();
    cb[nsub] = nch;
    // slots per chunk: the longest row's L and U counts
    int64_t nslot = 0;
    for (int64_t c = 0; c < nch; ++c) {
        offl.push_back(nslot);
        offu.push_back(nslot + nsl[c]);
        nslot += nsl[c] + nsu[c];
        G.slots_sub[csub[c]] += nsl[c] + nsu[c];
    }
    rowidx.assign(nch * kChunk, 0);
    const bool c16 = L.fits16;
    if (c16) G.col16.assign(std::max<int64_t>(nslot * kChunk, 1), 0);
    else G.col.assign(std::max<int64_t>(nslot * kChunk, 1), 0);
    G.val = BlockValues(vt, nslot, true);
#pragma omp parallel for schedule(dynamic, 64)
    for (int64_t c = 0; c < nch; ++c) {
        const auto& R = rows[lists[c]];
        const int k = (int)(lists[c] % KG);
        const int64_t r0 = base[c], nr = std::min<int64_t>(kChunk, (int64_t)R.size() - r0);
        for (int64_t lane = 0; lane < kChunk; ++lane) {
            const bool real = lane < nr;
            const int64_t g = real ? R[r0 + lane] : R[r0];
            rowidx[c * kChunk + lane] = real ? (int32_t)g : ~(int32_t)g;
            // pad slots: the row itself (offset 0), zero blocks
            for (int64_t q = offl[c]; q < offl[c] + nsl[c] + nsu[c]; ++q) {
                if (c16) G.col16[q * kChunk + lane] = 0;
                else G.col[q * kChunk + lane] = (int32_t)g;
            }
            if (!real) continue;
            const int64_t nc = g / kChunk, nl = g % kChunk;
            int64_t ql = offl[c], qu = offu[c];
            for (int64_t q = off[nc]; q < off[nc + 1]; ++q) {
                const int64_t j = col[q * kChunk + nl];
                if (j == g) continue;
                const int st = store(k, j);
                if (st < 0) continue;
                const int64_t t = st == 0 ? ql++ : qu++;
                if (c16) G.col16[t * kChunk + lane] = (int16_t)(j - g);
                else G.col[t * kChunk + lane] = (int32_t)j;
                G.val.put(t, lane, &val[q * 9 * kChunk + nl], kChunk);
            }
        }
    }
    if (!G.val.ok) throw ApiError(DDPCA_EINVAL, "block-scaled int8 copy: a block's scale is out of fp32's normal range");
    // the byte model's counts: per colour the rows, the L and U blocks, and every distinct x entry
    // a launch gathers (forward colour k: rows of earlier colours; residual: later ones; backward:
    // all other colours) once
    {
        std::vector<double> nl_k(K, 0.0), nu_k(K, 0.0), rows_k(K, 0.0), gx_f(K, 0.0), gx_b(K, 0.0);
        double gx_r = 0.0;
        std::vector<int32_t> seen_f(L.nn, -1), seen_b(L.nn, -1), seen_r(L.nn, 0), seen_u(L.nn, -1), seen_l(L.nn, 0);
        std::vector<double> gx_u(K, 0.0);
        double gx_l = 0.0;
        for (int k = 0; k < K; ++k)
            for (int s = 0; s < nsub; ++s)
                for (int64_t g : rows[(size_t)s * KG + k]) {
                    rows_k[k] += 1.0;
                    const int64_t nc = g / kChunk, lane = g % kChunk;
                    for (int64_t q = off[nc]; q < off[nc + 1]; ++q) {
                        const int64_t j = col[q * kChunk + lane];
                        if (j == g) continue;
                        if (colour[j] < k) {
                            nl_k[k] += 1.0;
                            if (seen_f[j] != k) seen_f[j] = k, gx_f[k] += 1.0;
                            if (!seen_l[j]) seen_l[j] = 1, gx_l += 1.0;
                        } else {
                            nu_k[k] += 1.0;
                            if (!seen_r[j]) seen_r[j] = 1, gx_r += 1.0;
                            if (seen_u[j] != k) seen_u[j] = k, gx_u[k] += 1.0;
                        }
                        if (seen_b[j] != k) seen_b[j] = k, gx_b[k] += 1.0;
                    }
                }
        G.gx_f = gx_f;
        G.gx_b = gx_b;
        G.rows_k = rows_k;
        G.gx_r = gx_r;
        G.gx_u = gx_u;
        G.gx_l = gx_l;
        G.nl_k = nl_k;
        G.nu_k = nu_k;
        G.vb = vbytes(vt) + (c16 ? 2.0 : 4.0);
        G.rowf = 24.0 + (vt == kVal64 ? 72.0 : 36.0) + 24.0 + 4.0;
    }
    G.ncol = K;
    G.nchunk = nch;
    G.first.assign(KG, 0);
    G.count.assign(KG, 0);
    for (int k = 0; k < KG; ++k) {
        G.first[k] = (int64_t)G.list.size();
        G.count[k] = (int64_t)bycol[k].size();
        G.list.insert(G.list.end(), bycol[k].begin(), bycol[k].end());
    }
    colour_byte_model(G, 3, false, false);
    if (vt != kVal64 && minv32) {
        const std::vector<float>& m32 = *minv32;
        G.minvc.assign((size_t)nch * 9 * kChunk, 0.0f);
#pragma omp parallel for schedule(static)
        for (int64_t c = 0; c < nch; ++c)
            for (int64_t lane = 0; lane < kChunk; ++lane) {
                const int32_t rr = rowidx[c * kChunk + lane];
                const int64_t g = rr >= 0 ? rr : ~rr;  // pad lanes: the chunk's first row (their x is not stored)
                for (int ij = 0; ij < 9; ++ij) G.minvc[(c * 9 + ij) * kChunk + lane] = m32[9 * g + ij];
            }
    }
    if (tune.verbose) {
        int64_t nb = 0, nr = 0, nf = 0;
        for (int s = 0; s < nsub; ++s) nb += G.band_rows_sub[s], nr += G.ring_rows_sub[s], nf += G.far_rows_sub[s];
        std::fprintf(stderr, "[ddpca] fine level: multicolour Gauss-Seidel, %d colours, %lld chunks, %lld slots%s\n", K,
                     (long long)nch, (long long)nslot,
                     band ? (", band " + std::to_string(nb) + " / ring " + std::to_string(nr) + " / far " + std::to_string(nf) + " rows").c_str() : "");
    }
    return G;
}

// Per launch: a block's stored value record + its column entry (vb), per real row b, the fp32
// inverse, x or r written and the row index (rowf), and every distinct x entry the launch gathers
void colour_byte_model(ColourShape& G, int smoother, bool x4, bool r4) {
    const int K = G.ncol;
    std::vector<double> lb;
    if (smoother == 4) {
        // k_gs_ssor's launch order: forward colours 0..K-1 (L), backward K-1..0 (U), the residual (L,
        // every chunk), forward 0..K-1 (L + U), backward K-1..0 (U); per row b, the fp32 inverse, w
        // and x as each phase moves them, x gathered once per distinct node
        const double xb = x4 ? 16.0 : 24.0, rb = r4 ? 16.0 : 24.0, m = 36.0, ix = 4.0;
        for (int k = 0; k < K; ++k) lb.push_back(G.vb * G.nl_k[k] + G.rows_k[k] * (24 + m + xb + 24 + ix) + xb * G.gx_f[k]);
        for (int k = K - 1; k >= 0; --k) lb.push_back(G.vb * G.nu_k[k] + G.rows_k[k] * (48 + m + xb + ix) + xb * G.gx_u[k]);
        double res = xb * G.gx_l;
        for (int k = 0; k < K; ++k) res += G.vb * G.nl_k[k] + G.rows_k[k] * (24 + rb + ix);
        lb.push_back(res);
        for (int k = 0; k < K; ++k)
            lb.push_back(G.vb * (G.nl_k[k] + G.nu_k[k]) + G.rows_k[k] * (24 + m + xb + 24 + ix) + xb * G.gx_b[k]);
        for (int k = K - 1; k >= 0; --k)
            lb.push_back(G.vb * G.nu_k[k] + G.rows_k[k] * (48 + m + 24 + (x4 ? xb : 0.0) + ix) + xb * G.gx_u[k]);
        G.launch_bytes = lb;
        return;
    }
    double res = 0.0;
    for (int k = 0; k < K; ++k) {
        lb.push_back(G.vb * G.nl_k[k] + G.rowf * G.rows_k[k] + 24.0 * G.gx_f[k]);
        res += G.vb * G.nu_k[k] + 28.0 * G.rows_k[k];
    }
    lb.push_back(res + 24.0 * G.gx_r);
    for (int k = K - 1; k >= 0; --k) lb.push_back(G.vb * (G.nl_k[k] + G.nu_k[k]) + G.rowf * G.rows_k[k] + 24.0 * G.gx_b[k]);
    if (x4) {
        // on the 16-B iterate: gathers 16 instead of 24 B per distinct node, the forward sweep writes
        // 16 B per row, the backward sweep 16 + 24; r4: the residual written in 16 B
        for (int k = 0; k < K; ++k) {
            lb[k] -= 8.0 * G.gx_f[k] + 8.0 * G.rows_k[k];
            lb[2 * K - k] += -8.0 * G.gx_b[k] + 16.0 * G.rows_k[k];
        }
        if (K) lb[K] -= 8.0 * G.gx_r;
        if (r4)
            for (int k = 0; k < K; ++k) lb[K] -= 8.0 * G.rows_k[k];
    }
    G.launch_bytes = lb;
}

// ============================================================================== coarse
int choose_coarse_level(const std::vector<SubdomainOps>& subs, int coarse_level_opt, int64_t* n0max) {
    const int nsub = (int)subs.size(), nlev = (int)subs[0].nnodes.size();
    int clev = 0;
    if (coarse_level_opt >= 0) clev = std::min(coarse_level_opt, nlev - 1);
    else
        for (int l = nlev - 2; l >= 1; --l) {
            double bytes = 0.0;
            int64_t nmax = 0;
            for (int s = 0; s < nsub; ++s) {
                const double n = 3.0 * (double)subs[s].nnodes[l];
                bytes += 8.0 * n * n;
                nmax = std::max<int64_t>(nmax, 3 * subs[s].nnodes[l]);
            }
            if (bytes <= 256.0 * 1024 * 1024 && nmax <= 12288) { clev = l; break; }
        }
    if (nlev > 1 && clev == nlev - 1) clev = nlev - 2;
    *n0max = 0;
    for (int s = 0; s < nsub; ++s) *n0max = std::max<int64_t>(*n0max, 3 * subs[s].nnodes[clev]);
    return clev;
}

std::vector<double> coarse_dense(const SubdomainOps& S, int clev, const std::vector<int32_t>& p, bool general) {
    const Bsr3& A = *S.K[clev];
    const uint8_t* fr = S.free_flags(clev);
    const int64_t nc = S.nnodes[clev], n0 = 3 * nc;
    std::vector<double> D(n0 * n0, 0.0);
    // a constrained dof's decoupled row and column (zeroed again after the inverse) carry 1,
    // or in the general path the largest free diagonal entry, so that its pivot does not
    // read as near-singular against stiffness-scaled ones (the LU inverse's pivot test)
    double cdiag = 1.0;
    if (general) {
        cdiag = 0.0;
        for (int64_t r = 0; r < nc; ++r)
            for (int64_t k = A.ptr[r]; k < A.ptr[r + 1]; ++k)
                if (A.col[k] == r)
                    for (int a = 0; a < 3; ++a)
                        if (fr[3 * r + a]) cdiag = std::max(cdiag, std::abs(A.val[9 * k + 4 * a]));
        if (!(cdiag > 0.0)) cdiag = 1.0;
    }
    for (int64_t r = 0; r < nc; ++r)
        for (int64_t k = A.ptr[r]; k < A.ptr[r + 1]; ++k) {
            const int64_t j = A.col[k];
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) {
                    double v = A.val[9 * k + 3 * a + b];
                    if (!fr[3 * r + a] || !fr[3 * j + b]) v = (j == r && a == b) ? cdiag : 0.0;
                    D[(3 * p[r] + a) * n0 + 3 * p[j] + b] = v;
                }
        }
    return D;
}

int64_t coarse_pack(std::vector<double>& D, const SubdomainOps& S, int clev, const std::vector<int32_t>& p,
                    int64_t padded_nodes, std::vector<double>& packed) {
    const uint8_t* fr = S.free_flags(clev);
    const int64_t nc = S.nnodes[clev], n0 = 3 * nc;
    for (int64_t r = 0; r < nc; ++r)
        for (int a = 0; a < 3; ++a) {
            if (fr[3 * r + a]) continue;
            const int64_t d = 3 * p[r] + a;
            for (int64_t e = 0; e < n0; ++e) D[d * n0 + e] = D[e * n0 + d] = 0.0;
        }
    const int64_t ld = (n0 + 3) / 4 * 4;  // rows padded for 16-B loads (k_coarse)
    if (ld > 3 * padded_nodes) throw ApiError(DDPCA_ESTATE, "coarse row padding beyond the member");
    for (int64_t r = 0; r < n0; ++r) {
        packed.insert(packed.end(), D.begin() + r * n0, D.begin() + (r + 1) * n0);
        packed.insert(packed.end(), ld - n0, 0.0);
    }
    return ld;
}

}  // namespace ddpca
