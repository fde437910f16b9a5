/* csrc/true_peak_taps.h on the host, under AddressSanitizer and UBSan (tests/test_true_peak_host.py): the 3 x 24 taps, the copy into a
 * caller's room and its refusals, and the range of intervals a block evaluates for every length from 0 to 30 and for 8192.  No device, no
 * context.
 *   true_peak_check [LEN...]   "OK", the 72 taps as hexadecimal floats, then "len:first:count" for every length given */
#include "true_peak_taps.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

int main(int argc, char **argv) {
    gdg_true_peak_table t;
    true_peak_build(&t);
    const double ulp = 2.220446049250313e-16;
    for (int p = 0; p < GDG_TRUE_PEAK_PHASES; p++) {
        double sum = 0.0;
        for (int k = 0; k < GDG_TRUE_PEAK_TAPS; k++) sum += t.h[p][k];
        CHECK(fabs(sum - 1.0) <= 24 * ulp);
        /* the two taps next to the point are the large ones, everything else is below them */
        for (int k = 0; k < GDG_TRUE_PEAK_TAPS; k++) CHECK(fabs(t.h[p][k]) <= 1.0 && (k == GDG_TRUE_PEAK_H - 1 || k == GDG_TRUE_PEAK_H || fabs(t.h[p][k]) < 0.25));
    }
    for (int k = 0; k < GDG_TRUE_PEAK_TAPS; k++) {
        CHECK(fabs(t.h[0][k] - t.h[2][GDG_TRUE_PEAK_TAPS - 1 - k]) <= 24 * ulp);          /* phase 1 mirrors phase 3 */
        CHECK(fabs(t.h[1][k] - t.h[1][GDG_TRUE_PEAK_TAPS - 1 - k]) <= 24 * ulp);          /* phase 2 is symmetric */
    }
    CHECK(fabs(t.h[1][GDG_TRUE_PEAK_H - 1] - 0.633825) < 1e-6);                            /* an impulse's half-way neighbours */
    /* the copy: exactly 72 entries, nothing behind them; refusals */
    std::vector<double> room(72, -7.0);
    CHECK(true_peak_copy(&t, room.data(), 72) && room[0] == t.h[0][0] && room[24] == t.h[1][0] && room[71] == t.h[2][23]);
    std::vector<double> wide(80, -7.0);
    CHECK(true_peak_copy(&t, wide.data(), 80) && wide[71] == t.h[2][23] && wide[72] == -7.0 && wide[79] == -7.0);
    std::vector<double> few(71, -7.0);
    CHECK(!true_peak_copy(&t, few.data(), 71) && few[0] == -7.0 && few[70] == -7.0);
    CHECK(!true_peak_copy(&t, nullptr, 72) && !true_peak_copy(&t, room.data(), 0) && !true_peak_copy(&t, room.data(), -5));
    /* the evaluated range: every length from 0 to 30, and a whole block; every tap of every evaluated interval reads inside the block */
    for (size_t len = 0; len <= 8192; len = len < 30 ? len + 1 : (len == 30 ? 8192 : 8193)) {
        size_t first = 0, count = 0;
        true_peak_range(len, &first, &count);
        CHECK(first == 11 && count == (len >= 24 ? len - 23 : 0));
        std::vector<double> x(len, 0.5);                                                    /* ASan guards both ends */
        double worst = 0.0;
        for (size_t n = first; n < first + count; n++)
            for (int p = 0; p < GDG_TRUE_PEAK_PHASES; p++) {
                double acc = 0.0;
                for (int j = -GDG_TRUE_PEAK_H + 1; j <= GDG_TRUE_PEAK_H; j++) acc = acc + x[n + (size_t)(j + GDG_TRUE_PEAK_H - 1) - (size_t)(GDG_TRUE_PEAK_H - 1)] * t.h[p][j + GDG_TRUE_PEAK_H - 1];
                if (fabs(acc) > worst) worst = fabs(acc);
            }
        CHECK(count == 0 ? worst == 0.0 : (worst >= 0.5 * (1.0 - 24 * ulp) && worst <= 0.5 * (1.0 + 24 * ulp)));      /* a constant is reproduced */
    }
    if (failures) { printf("FAILED %d\n", failures); return 1; }
    printf("OK");
    for (int p = 0; p < GDG_TRUE_PEAK_PHASES; p++)
        for (int k = 0; k < GDG_TRUE_PEAK_TAPS; k++) printf(" %a", t.h[p][k]);
    for (int i = 1; i < argc; i++) {
        size_t first = 0, count = 0;
        const size_t len = (size_t)strtoull(argv[i], nullptr, 10);
        true_peak_range(len, &first, &count);
        printf(" %zu:%zu:%zu", len, first, count);
    }
    printf("\n");
    return 0;
}
