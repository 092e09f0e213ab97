// CPU build of the request kernels' index helpers (csrc/dh_index.h) against plain `/` and `%`,
// over the whole domain each helper is used on (tests/test_index_helpers.py).  Every function
// returns the number of mismatches.
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <thread>
#include <vector>

#include "dh_index.h"

namespace {

template <int RT>
int64_t group_mismatches(unsigned* r_seen) {
    int64_t bad = 0;
    for (int nopt = 0; nopt <= 256; ++nopt) {
        const int R = std::min(RT, std::max(nopt, 1));
        *r_seen |= 1u << R;
        bad += dh_idx::group_r<RT>(nopt) != R;
        bad += dh_idx::n_groups<RT>(nopt) != (nopt + R - 1) / R;
        for (int oi = 0; oi < nopt; ++oi) {
            bad += dh_idx::opt_group<RT>(oi, nopt) != oi / R;
            bad += dh_idx::opt_slot<RT>(oi, nopt) != oi % R;
        }
    }
    return bad;
}

// values qt of [lo, hi) against 64-bit division
int64_t table_range(int64_t lo, int64_t hi, int tpp) {
    int64_t bad = 0;
    for (int64_t qt = std::max<int64_t>(lo, 0); qt < hi; ++qt) {
        int64_t p;
        int g;
        dh_idx::table_split(qt, tpp, p, g);
        bad += p != qt / tpp || g != (int)(qt % tpp);
    }
    return bad;
}

// m * tpp - 1, m * tpp, m * tpp + 1 for the multiples m in [m0, m1), none above 2^31 - 1; the
// expected pairs follow from m, with no division
int64_t table_multiples(int64_t m0, int64_t m1, int tpp) {
    const int64_t top = (int64_t(1) << 31) - 1;
    int64_t bad = 0;
    for (int64_t m = m0; m < m1; ++m) {
        const int64_t base = m * tpp;
        int64_t p;
        int g;
        if (base >= 1) {
            dh_idx::table_split(base - 1, tpp, p, g);
            bad += p != m - 1 || g != tpp - 1;
        }
        dh_idx::table_split(base, tpp, p, g);
        bad += p != m || g != 0;
        if (base + 1 <= top) {
            dh_idx::table_split(base + 1, tpp, p, g);
            bad += tpp == 1 ? (p != m + 1 || g != 0) : (p != m || g != 1);
        }
    }
    return bad;
}

}  // namespace

extern "C" {

// t in [0, 256) and the tile widths 64, 128, 256 by G in [1, 256]; the staging rotation for every
// block size of whole waves
int64_t dh_idx_lane_mismatches() {
    int64_t bad = 0;
    for (unsigned G = 1; G <= 256; ++G) {
        const unsigned m = dh_idx::div256_magic(G);
        for (unsigned x = 0; x <= 256; ++x) {
            const unsigned q = dh_idx::div256(x, m);
            bad += q != x / G;
            bad += dh_idx::mod256(x, q, G) != x % G;
        }
    }
    for (int n = 64; n <= 1024; n += 64)
        for (int t = 0; t < n; ++t) bad += dh_idx::rot64(t, n) != (t + n - 64) % n;
    return bad;
}

// R = min(RT, max(nopt, 1)) for RT in {1, 2, 4} and nopt in [0, 256], every option index below
// nopt; *r_seen gets bit R set for every R met
int64_t dh_idx_group_mismatches(unsigned* r_seen) {
    *r_seen = 0;
    return group_mismatches<1>(r_seen) + group_mismatches<2>(r_seen) + group_mismatches<4>(r_seen);
}

// tpp in [1, 4096]: the first and last 4,096 values below tpp * 2^k for every k that keeps them
// below 2^31, and the three values around every multiple of tpp up to 2^31 - 1 (5.7e10 values:
// spread over n_threads)
int64_t dh_idx_table_mismatches(int n_threads) {
    const int64_t lim = int64_t(1) << 31;
    constexpr int64_t kChunk = int64_t(1) << 22;          // multiples per work item
    struct Item { int tpp; int64_t m0, m1; };
    std::vector<Item> items;
    for (int tpp = 1; tpp <= 4096; ++tpp) {
        const int64_t n_mult = (lim - 1) / tpp + 1;       // multiples 0 .. floor((2^31 - 1) / tpp)
        for (int64_t m0 = 0; m0 < n_mult; m0 += kChunk)
            items.push_back({tpp, m0, std::min(m0 + kChunk, n_mult)});
    }
    std::atomic<size_t> next{0};
    std::atomic<int64_t> bad{0};
    auto work = [&] {
        int64_t b = 0;
        for (size_t i; (i = next.fetch_add(1)) < items.size();)
            b += table_multiples(items[i].m0, items[i].m1, items[i].tpp);
        bad += b;
    };
    std::vector<std::thread> th;
    for (int i = 1; i < std::max(n_threads, 1); ++i) th.emplace_back(work);
    for (int tpp = 1; tpp <= 4096; ++tpp) {
        int64_t b = table_range(0, std::min<int64_t>(4096, lim), tpp);
        for (int k = 0; (int64_t(tpp) << k) <= lim; ++k) {
            const int64_t end = int64_t(tpp) << k;
            b += table_range(end - 4096, end, tpp);
        }
        bad += b;
    }
    work();
    for (auto& t : th) t.join();
    return bad.load();
}

}  // extern "C"
