// Value layout of the streamed SELL-BSR3 operators of MGPIS: what one slot (64 lanes x one 3x3
// block) looks like in each storage type, and the host-side packing of a block into it.  Read by
// the kernels (device_mgpis*.hip) and by the host plan (mgpis_plan.cpp), so it is plain C++: the
// __host__ __device__ qualifiers sit behind DDPCA_HD and nothing here needs the HIP headers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>

#ifdef __HIPCC__
#define DDPCA_HD __host__ __device__
#else
#define DDPCA_HD
#endif

namespace ddpca {

constexpr int kChunk = 64;  // SELL chunk = one node row per lane of a wave
inline int64_t pad64(int64_t n) { return (n + 63) / 64 * 64; }

// Storage type of streamed operator values (arithmetic is fp64 throughout).
enum ValType { kVal64 = 0, kVal32 = 1, kValH16 = 2, kValQ8 = 3 };  // H16: block-exponent fp16, Q8: block-scaled int8

// fp64, paired (DDPCA_PAIRED_VALUES = 1, default): 16-B lane loads -- four 1-KiB wave runs of
// (v[2p], v[2p+1]), then a 512-B run of v[8]: 5 load instructions per block instead of 9, the
// fine PCG SpMV 5-8 % faster (profiles/r01_spmv_ab.json).  fp32 keeps nine 256-B runs, one per
// entry: its paired forms -- two 16-B quads + v[8], or four 8-B pairs + v[8] -- measured 4-13 %
// SLOWER in the smoothing and residual kernels (profiles/r01_spmv_ab.json, _f32pairs.json).  Element (ij, lane) of slot base sb:
//   paired fp64: sb[(ij < 8 ? 128 * (ij / 2) + 2 * lane + ij % 2 : 512 + lane)]
//   otherwise:   sb[ij * 64 + lane]
#ifndef DDPCA_PAIRED_VALUES
#define DDPCA_PAIRED_VALUES 1
#endif
template <typename T>
constexpr bool paired_values() { return DDPCA_PAIRED_VALUES != 0 && sizeof(T) == 8; }

template <typename T>
DDPCA_HD inline int64_t slot_elem(int ij, int64_t lane) {
    if (!paired_values<T>()) return (int64_t)ij * kChunk + lane;
    return ij == 8 ? 512 + lane : 128 * (ij / 2) + 2 * lane + ij % 2;
}

// Block-exponent fp16 storage (T = uint16_t; precond_fp32 = 2, the fine level's V-cycle copy):
// each 3x3 block is 2^e times nine fp16 values, e = the binary exponent of the block's largest
// |entry| (so |values| < 1 and every entry within 2^14 of the block maximum keeps fp16's 11
// significant bits); the record is ten halves, (v0,v1) (v2,v3) (v4,v5) (v6,v7) (v8,e), one
// 256-B dword run per pair: a slot is 1280 B, 20 B per block against 36 B for fp32.  A block
// and its transpose share e and round alike, so the operator stays exactly symmetric.
//
// Block-scaled int8 storage (T = uint8_t; precond_fp32 = 3): nine int8 values times a per-block
// scale max|entry| / 127 kept to 16 mantissa bits (the fp32 scale's top 24 bits, the low byte of
// its word holds q8), so the largest entry maps to 127 and every entry is within half a scale of
// its value; the record is three 256-B dword runs per slot, (q0..q3) (q4..q7) (q8 | scale bits
// 8..31): 12 B per block against 20 for fp16.  Symmetric as the fp16 copy (a block and its
// transpose share the scale).  With the Krylov operator and the stop rule in fp64 only the
// preconditioner moves: 18-19 PCG iterations per solve against 18 with the fp16 copy, the
// headline +5.7 % (a power-of-two scale, 10 B per block, took 19-20 and +4.0 %).
template <typename T>
constexpr int slot_vals() { return sizeof(T) == 1 ? 12 : sizeof(T) == 2 ? 10 : 9; }
// the same by ValType: stored elements of one block, and their bytes
inline int vals_per_block(int vt) { return vt == kValQ8 ? 12 : vt == kValH16 ? 10 : 9; }
inline double vbytes(int vt) { return vt == kValQ8 ? 12.0 : vt == kValH16 ? 20.0 : vt == kVal32 ? 36.0 : 72.0; }

// position of record half k (0..9) of `lane` in a 1280-B fp16 slot, of record byte k (0..11) in
// a 768-B int8 slot
inline int64_t h16_pos(int k, int64_t lane) { return 128 * (k / 2) + 2 * lane + k % 2; }
inline int64_t q8_pos(int k, int64_t lane) { return 256 * (k / 4) + 4 * lane + k % 4; }

// double -> IEEE half, round to nearest even in one rounding, in integer arithmetic: the host
// compilers of this library do not all have _Float16, and the stored bytes must not depend on
// which one built the plan (tests/test_h16_convert.py sets it against clang's conversion)
inline uint16_t f64_to_h16(double x) {
    const uint64_t b = __builtin_bit_cast(uint64_t, x);
    const uint16_t sign = (uint16_t)((b >> 48) & 0x8000u);
    const int e = (int)((b >> 52) & 0x7FF);
    uint64_t m = b & 0xFFFFFFFFFFFFFull;
    if (e == 0x7FF) return (uint16_t)(sign | 0x7C00u | (m ? 0x200u | (uint16_t)(m >> 42) : 0u));
    const int he = e - 1023 + 15;  // the half's biased exponent
    if (he >= 31) return (uint16_t)(sign | 0x7C00u);
    if (e == 0 || he < -11) return sign;  // below half of the smallest subnormal half
    m |= 1ull << 52;
    // normal halves drop 42 bits of the 53-bit significand (whose leading one then adds the last
    // unit of the exponent field), subnormal ones 43 - he
    const int shift = he >= 1 ? 42 : 43 - he;
    uint64_t q = m >> shift;
    const uint64_t rem = m & ((1ull << shift) - 1), half = 1ull << (shift - 1);
    if (rem > half || (rem == half && (q & 1))) ++q;  // a carry runs into the exponent: next binade, or inf
    return (uint16_t)(sign | (uint16_t)(((uint64_t)(he >= 1 ? he - 1 : 0) << 10) + q));
}

// host: one block (9 fp64 entries, row-major) -> the ten-half record
inline void to_h16_block(const double* v, uint16_t* rec) {
    double m = 0.0;
    for (int k = 0; k < 9; ++k) m = std::max(m, std::fabs(v[k]));
    int e = 0;
    if (m > 0.0) std::frexp(m, &e);
    for (int k = 0; k < 9; ++k) rec[k] = f64_to_h16(std::ldexp(v[k], -e));
    rec[9] = (uint16_t)(int16_t)e;
}

// host: one block -> the twelve-byte int8 record (nine values, then the scale's bits 8..31); false
// when the block is outside the range the reduced-precision copies are specified for: an entry
// beyond fp32's largest number (3.4e38), or a scale below fp32's normal range (entries below ~1e-36)
inline bool to_q8_block(const double* v, uint8_t* rec) {
    double m = 0.0;
    for (int k = 0; k < 9; ++k) m = std::max(m, std::fabs(v[k]));
    if (m > (double)std::numeric_limits<float>::max()) return false;
    const float s32 = (float)(m / 127.0);
    if (m > 0.0 && !(s32 > 0.0f && std::isfinite(s32) && std::isnormal(s32))) return false;
    const uint32_t bits = __builtin_bit_cast(uint32_t, s32) & 0xFFFFFF00u;
    const double sc = (double)__builtin_bit_cast(float, bits);
    for (int k = 0; k < 9; ++k)
        rec[k] = (uint8_t)(int8_t)(sc > 0.0 ? std::max(-127.0, std::min(127.0, std::nearbyint(v[k] / sc))) : 0.0);
    rec[9] = (uint8_t)(bits >> 8);
    rec[10] = (uint8_t)(bits >> 16);
    rec[11] = (uint8_t)(bits >> 24);
    return true;
}

}  // namespace ddpca
