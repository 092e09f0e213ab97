// Index arithmetic of the request kernels' tiles: exact replacements for the integer divisions and
// modulos by block-uniform runtime values that every wave of a block used to expand in VALU.
// Plain C++ for host and device, so tests/native/idx_host.cpp checks each helper against `/` and
// `%` over its whole domain on the CPU (tests/test_index_helpers.py).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define DH_IDX __host__ __device__ __forceinline__
#else
#define DH_IDX inline
#endif

namespace dh_idx {

// (t + n - 64) % n for 0 <= t < n, n >= 64: the staging order "waves 1, 2, .., then wave 0"
DH_IDX int rot64(int t, int n) { return t >= 64 ? t - 64 : t + n - 64; }

// Division of x in [0, 256] by G in [1, 256] as a 24-bit multiply and a shift.  m = floor(2^16 / G)
// + 1 exceeds 2^16 / G by e in (0, 1], so x * m / 2^16 = x / G + x * e / 2^16, and x * e * G <=
// 256 * 256 = 2^16 with equality only where x / G is whole: the floor is never carried over.
// x * m <= 256 * 65537 < 2^32, and both factors are below 2^24.
DH_IDX unsigned div256_magic(unsigned G) { return 65536u / G + 1u; }
DH_IDX unsigned div256(unsigned x, unsigned m) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(x, m) >> 16;
#else
    return (x * m) >> 16;
#endif
}
// x % G from the quotient q = div256(x, m)
DH_IDX unsigned mod256(unsigned x, unsigned q, unsigned G) {
#if defined(__HIP_DEVICE_COMPILE__)
    return x - __umul24(q, G);
#else
    return x - q * G;
#endif
}

// Options per lane group, R = min(RT, max(nopt, 1)) with RT a power of two, and the divisions by
// it.  R < RT only where the tile has fewer than RT options, and then R = nopt (or 1 with none):
// the tile is one group, every option index oi < nopt is its own remainder and the quotient is 0.
template <int RT>
DH_IDX int group_r(int nopt) { return nopt < RT ? (nopt > 1 ? nopt : 1) : RT; }
template <int RT>
constexpr int log2_rt() {
    static_assert(RT > 0 && (RT & (RT - 1)) == 0, "RT is a power of two");
    int s = 0;
    while ((1 << s) < RT) ++s;
    return s;
}
// (nopt + R - 1) / R, nopt >= 0
template <int RT>
DH_IDX int n_groups(int nopt) {
    return nopt >= RT ? (nopt + RT - 1) >> log2_rt<RT>() : (nopt > 0 ? 1 : 0);
}
// oi / R and oi % R for 0 <= oi < nopt
template <int RT>
DH_IDX int opt_group(int oi, int nopt) { return nopt >= RT ? oi >> log2_rt<RT>() : 0; }
template <int RT>
DH_IDX int opt_slot(int oi, int nopt) { return nopt >= RT ? oi & (RT - 1) : oi; }

// Table qt = p * tpp + g of a fused grid as (p, g).  Grids have fewer than 2^31 blocks, so the
// 32-bit unsigned division gives what the split path's 64-bit one gives.
DH_IDX void table_split(int64_t qt, int tpp, int64_t& p, int& g) {
    p = (int64_t)((unsigned)qt / (unsigned)tpp);
    g = (int)((unsigned)qt % (unsigned)tpp);
}

}  // namespace dh_idx
