// The tap tables of the proton resampler (vent_analysis_amd/csrc/resample_host.h, the header the library
// includes) over a grid of maps: at most 8 taps, the in-range taps contiguous and inside the source, the
// weights > 0 in the used slots and 0 after them, the known tables of the identity and of scale 2, and the
// refusals.  Built with -fsanitize=address,undefined by tests/test_resample_taps.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "resample_host.h"

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            abort();                                                          \
        }                                                                     \
    } while (0)

struct Table {
    std::vector<int32_t> first, count;
    std::vector<float> weight;
    explicit Table(int64_t n) : first(n, -7), count(n, -7), weight(RS_TAPS * n, -7.0f) {}
};

static long sweep(int64_t n_src, int64_t n_dst) {
    const double scales[] = {0.25, 0.5, 0.6, 1.0, 1.3, 1.7, 2.0, 3.9, 4.0};
    const double offsets[] = {0.0, 0.5, -0.4, 2.0, -7.25, (double)n_src + 6.0, -1048576.0, 1048576.0};
    long used = 0;
    for (double s : scales)
        for (double o : offsets) {
            Table t(n_dst);
            CHECK(rs_axis_taps(n_src, n_dst, s, o, t.first.data(), t.count.data(), t.weight.data()));
            const double w = s > 1.0 ? s : 1.0;
            for (int64_t i = 0; i < n_dst; ++i) {
                const int32_t f = t.first[i], c = t.count[i];
                const float *wt = t.weight.data() + RS_TAPS * i;
                CHECK(c >= 0 && c <= RS_TAPS);
                CHECK(f >= 0 && (int64_t)f + c <= n_src);
                if (c == 0) CHECK(f == 0);
                double sum = 0.0;
                for (int k = 0; k < RS_TAPS; ++k) {
                    if (k < c) CHECK(wt[k] > 0.0f && wt[k] <= 1.0f);
                    else CHECK(wt[k] == 0.0f && !std::signbit(wt[k]));
                    sum += wt[k];
                }
                CHECK(sum <= 1.0 + 1e-6);
                // every used tap lies strictly inside (u - w, u + w), and a tap the table leaves out at
                // either end of its run is outside the source or outside that interval
                const double u = s * (double)i + o;
                for (int k = 0; k < c; ++k) CHECK(std::fabs((double)(f + k) - u) < w);
                if (c > 0) {
                    CHECK(f == 0 || !(std::fabs((double)(f - 1) - u) < w));
                    CHECK((int64_t)f + c == n_src || !(std::fabs((double)(f + c) - u) < w));
                    // all taps inside the source: the weights are a partition of one
                    if (u - w >= 0.0 && u + w <= (double)(n_src - 1)) CHECK(std::fabs(sum - 1.0) <= 1e-6);
                }
                used += c;
            }
        }
    return used;
}

static void known_tables() {
    {   // the identity: one tap of weight 1.0
        Table t(9);
        CHECK(rs_axis_taps(9, 9, 1.0, 0.0, t.first.data(), t.count.data(), t.weight.data()));
        for (int i = 0; i < 9; ++i) CHECK(t.first[i] == i && t.count[i] == 1 && t.weight[RS_TAPS * i] == 1.0f);
    }
    {   // scale 2, offset 0.5: (0.125, 0.375, 0.375, 0.125) around 2 i + 0.5
        Table t(8);
        CHECK(rs_axis_taps(16, 8, 2.0, 0.5, t.first.data(), t.count.data(), t.weight.data()));
        for (int i = 1; i < 7; ++i) {
            const float *w = t.weight.data() + RS_TAPS * i;
            CHECK(t.first[i] == 2 * i - 1 && t.count[i] == 4);
            CHECK(w[0] == 0.125f && w[1] == 0.375f && w[2] == 0.375f && w[3] == 0.125f && w[4] == 0.0f);
        }
        CHECK(t.first[0] == 0 && t.count[0] == 3 && t.weight[0] == 0.375f && t.weight[2] == 0.125f);   // j = -1 dropped
    }
    {   // scale 4 at an integer coordinate: the two ends of the closed interval have t = 0 and are no taps
        Table t(3);
        CHECK(rs_axis_taps(64, 3, 4.0, 8.0, t.first.data(), t.count.data(), t.weight.data()));
        CHECK(t.first[1] == 9 && t.count[1] == 7 && t.weight[RS_TAPS + 3] == 0.25f);
    }
    {   // taps wholly outside: count 0, weights 0
        Table t(4);
        CHECK(rs_axis_taps(5, 4, 1.0, 11.0, t.first.data(), t.count.data(), t.weight.data()));
        for (int i = 0; i < 4; ++i) CHECK(t.count[i] == 0 && t.first[i] == 0 && t.weight[RS_TAPS * i] == 0.0f);
    }
}

static void refusals() {
    Table t(4);
    int32_t *f = t.first.data(), *c = t.count.data();
    float *w = t.weight.data();
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    CHECK(!rs_axis_taps(0, 4, 1.0, 0.0, f, c, w) && !rs_axis_taps(1025, 4, 1.0, 0.0, f, c, w));
    CHECK(!rs_axis_taps(4, 0, 1.0, 0.0, f, c, w) && !rs_axis_taps(4, (int64_t)RS_MAX_DST + 1, 1.0, 0.0, f, c, w));
    CHECK(!rs_axis_taps(4, 4, 0.2499, 0.0, f, c, w) && !rs_axis_taps(4, 4, 4.0001, 0.0, f, c, w));
    CHECK(!rs_axis_taps(4, 4, nan, 0.0, f, c, w) && !rs_axis_taps(4, 4, inf, 0.0, f, c, w) &&
          !rs_axis_taps(4, 4, -1.0, 0.0, f, c, w));
    CHECK(!rs_axis_taps(4, 4, 1.0, nan, f, c, w) && !rs_axis_taps(4, 4, 1.0, inf, f, c, w) &&
          !rs_axis_taps(4, 4, 1.0, 1048577.0, f, c, w) && !rs_axis_taps(4, 4, 1.0, -1048577.0, f, c, w));
    CHECK(!rs_axis_taps(4, 4, 1.0, 0.0, nullptr, c, w) && !rs_axis_taps(4, 4, 1.0, 0.0, f, nullptr, w) &&
          !rs_axis_taps(4, 4, 1.0, 0.0, f, c, nullptr));
    for (int i = 0; i < 4; ++i) CHECK(f[i] == -7 && c[i] == -7 && w[RS_TAPS * i] == -7.0f);   // nothing written
    CHECK(rs_map_in_limits(0.25, -1048576.0) && rs_map_in_limits(4.0, 1048576.0) && !rs_map_in_limits(nan, nan));
}

int main() {
    long used = 0;
    used += sweep(1, 12);
    used += sweep(5, 9);
    used += sweep(21, 41);
    used += sweep(83, 41);
    used += sweep(1024, 257);
    CHECK(used > 0);
    known_tables();
    refusals();
    printf("resample taps ok (%ld taps)\n", used);
    return 0;
}
