// The host side of the fine registration (vent_analysis_amd/csrc/register_maps_host.h, the header the
// library includes): the candidate list of one axis against the formula and its refusals, and the pick
// against a brute-force search over random and tied scores, NaN included.  Built with
// -fsanitize=address,undefined by tests/test_register_maps_check.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "register_maps_host.h"

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            abort();                                                          \
        }                                                                     \
    } while (0)

static long candidates() {
    const double factors[] = {0.94, 0.97, 1.0, 1.03, 1.06}, shifts[] = {-0.5, 0.0, 0.5};
    const double bases[][2] = {{2.0, 1.0}, {0.5, -0.25}, {1.3, 7.7}, {3.7, -1000.0}};
    const int64_t dims[] = {1, 9, 41, 128, 1 << 20};
    long n = 0;
    for (const auto &b : bases)
        for (int64_t nd : dims) {
            std::vector<double> out(2 * 15, -7.0);
            CHECK(rm_axis_candidates(b[0], b[1], nd, factors, 5, shifts, 3, out.data()));
            const double c = ((double)nd - 1.0) / 2.0;
            for (int fi = 0; fi < 5; ++fi)
                for (int si = 0; si < 3; ++si, ++n) {
                    const double *at = out.data() + 2 * (fi * 3 + si);
                    CHECK(at[0] == b[0] * factors[fi]);
                    volatile double one_f = 1.0 - factors[fi];
                    volatile double lever = c * one_f;
                    volatile double moved = lever + shifts[si];
                    volatile double in_src = b[0] * moved;
                    CHECK(at[1] == b[1] + in_src);
                    CHECK(rs_map_in_limits(at[0], at[1]));
                }
            CHECK(out[2 * 7] == b[0] && out[2 * 7 + 1] == b[1]);   // factor 1, shift 0: the base itself
        }
    return n;
}

static void candidate_refusals() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double one[] = {1.0}, zero[] = {0.0}, wide[] = {1.0, 2.5}, far[] = {0.0, 1e6}, bad[] = {nan}, off[] = {inf};
    double out[4] = {-7.0, -7.0, -7.0, -7.0};
    CHECK(!rm_axis_candidates(2.0, 1.0, 41, nullptr, 1, zero, 1, out) && !rm_axis_candidates(2.0, 1.0, 41, one, 1, nullptr, 1, out) &&
          !rm_axis_candidates(2.0, 1.0, 41, one, 1, zero, 1, nullptr));
    CHECK(!rm_axis_candidates(2.0, 1.0, 41, one, 0, zero, 1, out) && !rm_axis_candidates(2.0, 1.0, 41, one, 1, zero, 0, out));
    CHECK(!rm_axis_candidates(2.0, 1.0, 0, one, 1, zero, 1, out) &&
          !rm_axis_candidates(2.0, 1.0, (int64_t)RS_MAX_DST + 1, one, 1, zero, 1, out));
    CHECK(!rm_axis_candidates(2.0, 1.0, 41, wide, 2, zero, 1, out));     // the second entry's scale is 5
    CHECK(!rm_axis_candidates(2.0, 1.0, 41, one, 1, far, 2, out));       // the second entry's offset is past 2^20
    CHECK(!rm_axis_candidates(2.0, 1.0, 41, bad, 1, zero, 1, out) && !rm_axis_candidates(2.0, 1.0, 41, one, 1, off, 1, out));
    CHECK(!rm_axis_candidates(nan, 1.0, 41, one, 1, zero, 1, out) && !rm_axis_candidates(2.0, inf, 41, one, 1, zero, 1, out));
    for (double v : out) CHECK(v == -7.0);   // nothing written
    CHECK(rm_axis_candidates(4.0, 1048576.0, 41, one, 1, zero, 1, out) && out[0] == 4.0 && out[1] == 1048576.0);
}

// the pick by sorting keys: (score descending, distance, index)
static void brute(const std::vector<double> &s, const int32_t *count, const int32_t *h, int32_t *best) {
    best[0] = h[0]; best[1] = h[1]; best[2] = h[2];
    bool any = false;
    double top = 0.0;
    int dist = 0;
    size_t i = 0;
    for (int kz = 0; kz < count[2]; ++kz)
        for (int kr = 0; kr < count[0]; ++kr)
            for (int kc = 0; kc < count[1]; ++kc, ++i) {
                if (std::isnan(s[i])) continue;
                const int d = std::abs(kr - h[0]) + std::abs(kc - h[1]) + std::abs(kz - h[2]);
                if (!any || s[i] > top || (s[i] == top && d < dist)) {
                    any = true; top = s[i]; dist = d;
                    best[0] = kr; best[1] = kc; best[2] = kz;
                }
            }
}

static long picks() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const int32_t counts[][3] = {{1, 1, 1}, {3, 3, 1}, {17, 17, 5}, {2, 4, 2}, {5, 1, 3}, {1, 17, 1}};
    unsigned long long state = 12345;
    auto next = [&]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(state >> 40); };
    long n = 0;
    for (const auto &count : counts) {
        const size_t nc = (size_t)count[0] * count[1] * count[2];
        for (int round = 0; round < 40; ++round) {
            std::vector<double> s(nc);   // (exactly nc doubles: a read past the scores is an ASan error)
            const int levels = round % 4 == 0 ? 1 : round % 4 == 1 ? 3 : 1000;   // all tied, many ties, few
            for (double &v : s) {
                v = (double)(next() % levels);
                if (round % 5 == 4 && next() % 3 == 0) v = nan;
                if (round == 39) v = nan;
            }
            int32_t home[3] = {(int32_t)(next() % count[0]), (int32_t)(next() % count[1]), (int32_t)(next() % count[2])};
            const int32_t mid[3] = {(count[0] - 1) / 2, (count[1] - 1) / 2, (count[2] - 1) / 2};
            int32_t got[3] = {-7, -7, -7}, want[3];
            CHECK(rm_pick(s.data(), count, home, got));
            brute(s, count, home, want);
            CHECK(got[0] == want[0] && got[1] == want[1] && got[2] == want[2]);
            CHECK(rm_pick(s.data(), count, nullptr, got));
            brute(s, count, mid, want);
            CHECK(got[0] == want[0] && got[1] == want[1] && got[2] == want[2]);
            if (round == 39) CHECK(got[0] == mid[0] && got[1] == mid[1] && got[2] == mid[2]);   // nothing but NaN
            ++n;
        }
    }
    // the refusals: nothing written
    const int32_t ok[3] = {3, 3, 1}, big[3] = {3, 18, 1}, none[3] = {0, 3, 1}, deep[3] = {3, 3, 6};
    const int32_t out_of[3] = {3, 0, 0}, neg[3] = {0, -1, 0};
    std::vector<double> s(9, 0.0);
    int32_t got[3] = {-7, -7, -7};
    CHECK(!rm_pick(nullptr, ok, nullptr, got) && !rm_pick(s.data(), nullptr, nullptr, got) && !rm_pick(s.data(), ok, nullptr, nullptr));
    CHECK(!rm_pick(s.data(), big, nullptr, got) && !rm_pick(s.data(), none, nullptr, got) && !rm_pick(s.data(), deep, nullptr, got));
    CHECK(!rm_pick(s.data(), ok, out_of, got) && !rm_pick(s.data(), ok, neg, got));
    CHECK(got[0] == -7 && got[1] == -7 && got[2] == -7);
    CHECK(rm_count_in_limits(ok) && !rm_count_in_limits(big) && !rm_count_in_limits(nullptr));
    return n;
}

int main() {
    const long nc = candidates();
    candidate_refusals();
    const long np = picks();
    CHECK(nc > 0 && np > 0);
    printf("register maps host ok (%ld candidates, %ld picks)\n", nc, np);
    return 0;
}
