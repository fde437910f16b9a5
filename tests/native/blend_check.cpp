/* csrc/blend.h on the host, under AddressSanitizer and UBSan (tests/test_blend_host.py): the validation of a blend list, the rule by which a
 * list replaces the one in force, and the sum on the host -- the known answer of include/gdg.h, its sensitivity to the term order, and, given
 * a table made with the numpy restatement (tests/blend_ref.py), the bits of random sums.  No device, no context. */
#include "blend.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static unsigned long long bits(double v) { unsigned long long b; memcpy(&b, &v, 8); return b; }

/* table: per line the term count K, then K weights and K samples and the sum, all as hex bit patterns */
static int check_table(const char *path) {
    FILE *f = fopen(path, "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return -1; }
    int lines = 0, K = 0;
    while (fscanf(f, "%d", &K) == 1) {
        if (K < 1 || K > GDG_BLEND_MAX_TERMS) { fclose(f); return -1; }
        std::vector<double> w((size_t)K), x((size_t)K);
        std::vector<const double *> rows((size_t)K);
        std::vector<int> channel((size_t)K);
        unsigned long long b = 0;
        for (int k = 0; k < K; k++) { if (fscanf(f, "%llx", &b) != 1) { fclose(f); return -1; } memcpy(&w[(size_t)k], &b, 8); }
        for (int k = 0; k < K; k++) { if (fscanf(f, "%llx", &b) != 1) { fclose(f); return -1; } memcpy(&x[(size_t)k], &b, 8); rows[(size_t)k] = &x[(size_t)k]; channel[(size_t)k] = k; }
        if (fscanf(f, "%llx", &b) != 1) { fclose(f); return -1; }
        const double s = gdg_blend_sample(rows.data(), 0, channel.data(), w.data(), 0, K);
        if (s != s) { double want; memcpy(&want, &b, 8); CHECK(want != want); }      /* a NaN answers a NaN */
        else CHECK(bits(s) == b);
        lines++;
    }
    fclose(f);
    return lines;
}

int main(int argc, char **argv) {
    if (argc > 1) {
        const int lines = check_table(argv[1]);
        if (lines < 0 || failures) { printf("FAILED %d checks\n", failures); return 1; }
        printf("OK %d rows\n", lines);
        return 0;
    }
    int b = 0, k = 0;
    /* the known answer and its reverse: three rows of 1.0 */
    const double ones[4] = { 1.0, 1.0, 1.0, 1.0 };
    const double *rows3[3] = { ones, ones, ones };
    const int first2[3] = { 0, 3, 6 }, chan[6] = { 0, 1, 2, 2, 1, 0 };
    const double w[6] = { 0.1, 0.2, 0.3, 0.3, 0.2, 0.1 };
    CHECK(gdg_blend_check(2, first2, chan, w, nullptr, 3, &b, &k) == BLEND_OK && b == -1 && k == -1);
    double o0[4], o1[4];
    double *out[2] = { o0, o1 };
    gdg_blend_sum_host(rows3, 4, 2, first2, chan, w, out);
    for (int i = 0; i < 4; i++) { CHECK(o0[i] == 0.6000000000000001 && o1[i] == 0.6 && o0[i] != o1[i]); }
    /* one term, a channel named twice, a zero weight on an infinity */
    const double inf = std::numeric_limits<double>::infinity();
    const double a[2] = { 0.25, inf }, c[2] = { -3.0, 2.0 };
    const double *rows2[2] = { a, c };
    const int one_first[2] = { 0, 1 }, one_chan[1] = { 1 };
    const double one_w[1] = { -1.0 };
    double r0[2];
    double *out1[1] = { r0 };
    gdg_blend_sum_host(rows2, 2, 1, one_first, one_chan, one_w, out1);
    CHECK(r0[0] == 3.0 && r0[1] == -2.0);
    const int twice_first[2] = { 0, 3 }, twice_chan[3] = { 0, 1, 0 };
    const double twice_w[3] = { 0.0, 0.5, 2.0 };
    gdg_blend_sum_host(rows2, 2, 1, twice_first, twice_chan, twice_w, out1);
    CHECK(r0[0] == (0.0 * 0.25 + 0.5 * -3.0) + 2.0 * 0.25 && r0[1] != r0[1]);      /* 0 * inf is NaN, and stays one */
    /* every refusal */
    const int f_ok[3] = { 0, 2, 3 }, ch_ok[3] = { 0, 1, 2 };
    const double w_ok[3] = { 0.6, 0.4, -1.0 }, g_ok[2] = { 1.0, -0.5 };
    CHECK(gdg_blend_check(2, f_ok, ch_ok, w_ok, g_ok, 3, &b, &k) == BLEND_OK);
    CHECK(gdg_blend_check(0, nullptr, nullptr, nullptr, nullptr, 3, &b, &k) == BLEND_OK);
    CHECK(gdg_blend_check(-1, f_ok, ch_ok, w_ok, nullptr, 3, &b, &k) == BLEND_COUNT);
    CHECK(gdg_blend_check(GDG_BLEND_MAX_BLENDS + 1, f_ok, ch_ok, w_ok, nullptr, 3, &b, &k) == BLEND_COUNT);
    CHECK(gdg_blend_check(2, nullptr, ch_ok, w_ok, nullptr, 3, &b, &k) == BLEND_NULL);
    CHECK(gdg_blend_check(2, f_ok, nullptr, w_ok, nullptr, 3, &b, &k) == BLEND_NULL);
    CHECK(gdg_blend_check(2, f_ok, ch_ok, nullptr, nullptr, 3, &b, &k) == BLEND_NULL);
    const int f_empty[3] = { 0, 2, 2 }, f_down[3] = { 0, 2, 1 }, f_start[3] = { 1, 2, 3 };
    CHECK(gdg_blend_check(2, f_empty, ch_ok, w_ok, nullptr, 3, &b, &k) == BLEND_EMPTY && b == 1);
    CHECK(gdg_blend_check(2, f_down, ch_ok, w_ok, nullptr, 3, &b, &k) == BLEND_FIRST && b == 1);
    CHECK(gdg_blend_check(2, f_start, ch_ok, w_ok, nullptr, 3, &b, &k) == BLEND_FIRST && b == 0);
    {
        std::vector<int> ch33(34, 0);
        std::vector<double> w33(34, 1.0);
        const int f33[3] = { 0, 1, 34 }, f32[3] = { 0, 1, 33 };
        CHECK(gdg_blend_check(2, f33, ch33.data(), w33.data(), nullptr, 1, &b, &k) == BLEND_TERMS && b == 1);
        CHECK(gdg_blend_check(2, f32, ch33.data(), w33.data(), nullptr, 1, &b, &k) == BLEND_OK);      /* 32 terms, one channel 32 times */
    }
    const int ch_high[3] = { 0, 1, 3 }, ch_low[3] = { 0, -1, 2 };
    CHECK(gdg_blend_check(2, f_ok, ch_high, w_ok, nullptr, 3, &b, &k) == BLEND_CHANNEL && b == 1 && k == 0);
    CHECK(gdg_blend_check(2, f_ok, ch_low, w_ok, nullptr, 3, &b, &k) == BLEND_CHANNEL && b == 0 && k == 1);
    const double w_nan[3] = { 0.6, std::numeric_limits<double>::quiet_NaN(), -1.0 }, w_inf[3] = { 0.6, 0.4, -inf };
    CHECK(gdg_blend_check(2, f_ok, ch_ok, w_nan, nullptr, 3, &b, &k) == BLEND_WEIGHT && b == 0 && k == 1);
    CHECK(gdg_blend_check(2, f_ok, ch_ok, w_inf, nullptr, 3, &b, &k) == BLEND_WEIGHT && b == 1 && k == 0);
    const double g_bad[2] = { 1.0, inf };
    CHECK(gdg_blend_check(2, f_ok, ch_ok, w_ok, g_bad, 3, &b, &k) == BLEND_GAIN && b == 1 && k == -1);
    /* a refusal leaves the setting in force as it is; a good list replaces it whole; 0 blends: off */
    BlendSet set;
    CHECK(set.count() == 0 && set.unit_gains());
    CHECK(gdg_blend_replace(set, 2, f_ok, ch_ok, w_ok, g_ok, 3, &b, &k) == BLEND_OK && set.count() == 2 && set.terms() == 3 && !set.unit_gains());
    const BlendSet kept = set;
    CHECK(gdg_blend_replace(set, 2, f_ok, ch_high, w_ok, g_ok, 3, &b, &k) == BLEND_CHANNEL);
    CHECK(gdg_blend_replace(set, 2, f_empty, ch_ok, w_ok, g_ok, 3, &b, &k) == BLEND_EMPTY);
    CHECK(gdg_blend_replace(set, 2, f_ok, ch_ok, w_ok, g_bad, 3, &b, &k) == BLEND_GAIN);
    CHECK(set.first == kept.first && set.channel == kept.channel && set.weight == kept.weight && set.gain == kept.gain);
    CHECK(gdg_blend_replace(set, 1, one_first, one_chan, one_w, nullptr, 3, &b, &k) == BLEND_OK && set.count() == 1 && set.gain.size() == 1 && set.unit_gains());
    CHECK(gdg_blend_replace(set, 0, nullptr, nullptr, nullptr, nullptr, 3, &b, &k) == BLEND_OK && set.count() == 0 && set.terms() == 0);
    if (failures) { printf("FAILED %d checks\n", failures); return 1; }
    printf("OK\n");
    return 0;
}
