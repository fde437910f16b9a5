/* csrc/blend.h on the host, under AddressSanitizer and UBSan (tests/test_blend_delay_host.py): what gdg_blend_check refuses of a list with
 * delays and how such a list replaces the one in force, the delayed sum against the known answer of include/gdg.h (the first difference)
 * with and without a history, and the planner that turns alignment records into delays and signs -- the lower median, the threshold, a port
 * without a valid block, signs, and a blend of mixed references, which writes nothing.  No device, no context. */
#include "blend.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static gdg_blend_align_rec rec(double corr, double ref_sq, double sq, int lag) {
    gdg_blend_align_rec r;
    memset(&r, 0, sizeof r);
    r.corr = corr; r.corr0 = 0.0; r.ref_sq = ref_sq; r.sq_at_lag = sq; r.lag = lag;
    return r;
}

int main() {
    int b = 0, k = 0;
    /* ---- refusals of delays, and the list in force ---- */
    const int f_ok[3] = { 0, 2, 3 }, ch_ok[3] = { 0, 1, 2 };
    const double w_ok[3] = { 0.6, 0.4, -1.0 };
    const int d_ok[3] = { 0, GDG_BLEND_MAX_DELAY, 1 }, d_zero[3] = { 0, 0, 0 }, d_neg[3] = { 0, -1, 0 }, d_big[3] = { 0, 0, GDG_BLEND_MAX_DELAY + 1 };
    CHECK(gdg_blend_check(2, f_ok, ch_ok, w_ok, d_ok, nullptr, 3, &b, &k) == BLEND_OK && b == -1 && k == -1);
    CHECK(gdg_blend_check(2, f_ok, ch_ok, w_ok, (const int *)nullptr, nullptr, 3, &b, &k) == BLEND_OK);
    CHECK(gdg_blend_check(2, f_ok, ch_ok, w_ok, d_neg, nullptr, 3, &b, &k) == BLEND_DELAY && b == 0 && k == 1);
    CHECK(gdg_blend_check(2, f_ok, ch_ok, w_ok, d_big, nullptr, 3, &b, &k) == BLEND_DELAY && b == 1 && k == 0);
    const int ch_high[3] = { 0, 3, 2 };
    CHECK(gdg_blend_check(2, f_ok, ch_high, w_ok, d_neg, nullptr, 3, &b, &k) == BLEND_CHANNEL && b == 0 && k == 1);      /* the term's first offence */
    BlendSet set;
    CHECK(set.max_delay() == 0);
    CHECK(gdg_blend_replace(set, 2, f_ok, ch_ok, w_ok, d_ok, nullptr, 3, &b, &k) == BLEND_OK && set.count() == 2 && set.max_delay() == GDG_BLEND_MAX_DELAY && set.delay.size() == 3);
    /* first | channel | delay | pad | weight | gain: 3 + 3 + 3 ints padded to 40 bytes, 3 + 2 doubles */
    CHECK(set.packed_ints() == 40 && set.packed.size() == 40 + 5 * sizeof(double));
    { int d1 = -1; memcpy(&d1, set.packed.data() + 7 * sizeof(int), sizeof d1); CHECK(d1 == GDG_BLEND_MAX_DELAY); }
    { double w0 = 0.0; memcpy(&w0, set.packed.data() + 40, sizeof w0); CHECK(w0 == 0.6); }
    const BlendSet kept = set;
    CHECK(gdg_blend_replace(set, 2, f_ok, ch_ok, w_ok, d_big, nullptr, 3, &b, &k) == BLEND_DELAY);
    CHECK(set.delay == kept.delay && set.first == kept.first && set.weight == kept.weight && set.packed == kept.packed);
    /* all zeros: the list without delays, byte for byte */
    BlendSet plain, zeros;
    CHECK(gdg_blend_replace(plain, 2, f_ok, ch_ok, w_ok, nullptr, 3, &b, &k) == BLEND_OK);
    CHECK(gdg_blend_replace(zeros, 2, f_ok, ch_ok, w_ok, d_zero, nullptr, 3, &b, &k) == BLEND_OK);
    CHECK(zeros.max_delay() == 0 && zeros.delay.empty() && zeros.packed == plain.packed && plain.packed_ints() == 24);
    CHECK(gdg_blend_replace(set, 0, nullptr, nullptr, nullptr, (const int *)nullptr, nullptr, 3, &b, &k) == BLEND_OK && set.count() == 0 && set.max_delay() == 0);

    /* ---- the known answer: d = {0, 1}, weights {1, -1} on one row: the first difference ---- */
    const double x[6] = { 0.5, -0.25, 3.0, 3.0, -0.0, 1e-300 };
    const double *rows1[1] = { x };
    const int df[2] = { 0, 2 }, dch[2] = { 0, 0 }, dd[2] = { 0, 1 };
    const double dw[2] = { 1.0, -1.0 };
    double o[6];
    double *out1[1] = { o };
    gdg_blend_sum_host_delayed(rows1, nullptr, 6, 1, df, dch, dw, dd, out1);
    CHECK(o[0] == 0.5 && o[1] == -0.75 && o[2] == 3.25 && o[3] == 0.0 && o[4] == -3.0 && o[5] == 1e-300);
    std::vector<double> hist((size_t)GDG_BLEND_MAX_DELAY, 7.0);
    hist[(size_t)GDG_BLEND_MAX_DELAY - 1] = 2.0;                              /* sample -1 */
    hist[0] = -4.0;                                                          /* sample -4096 */
    const double *h1[1] = { hist.data() };
    gdg_blend_sum_host_delayed(rows1, h1, 6, 1, df, dch, dw, dd, out1);
    CHECK(o[0] == -1.5 && o[1] == -0.75);
    const int dmax[2] = { 0, GDG_BLEND_MAX_DELAY };
    gdg_blend_sum_host_delayed(rows1, h1, 6, 1, df, dch, dw, dmax, out1);
    CHECK(o[0] == 4.5 && o[1] == -7.25 && o[5] == 1e-300 - 7.0);             /* the oldest sample of the history, then the next ones */
    gdg_blend_sum_host_delayed(rows1, nullptr, 6, 1, df, dch, dw, nullptr, out1);
    for (int i = 0; i < 6; i++) CHECK(o[i] == 0.0);                          /* no delay: x - x */
    /* a negative weight in front of the job: the product is -0.0, and +0.0 + -0.0 is +0.0 */
    const double z[2] = { 0.0, 1.0 };
    const double *rowsz[1] = { z };
    gdg_blend_sum_host_delayed(rowsz, nullptr, 2, 1, df, dch, dw, dd, out1);
    CHECK(o[0] == 0.0 && !std::signbit(o[0]) && o[1] == 1.0);

    /* ---- the planner ---- */
    /* 4 ports, 5 blocks: ports 1 and 2 measured against 0, port 3 against itself */
    const int ref[4] = { -1, 0, 0, 3 };
    std::vector<gdg_blend_align_rec> R(4 * 5, rec(0, 0, 0, 0));
    /* port 1: lags {37, 37, 36, 900 (weak), 38}: the weak block is below the threshold; lower median of {36, 37, 37, 38} = 37; corr negative */
    R[5 + 0] = rec(-9.0, 10.0, 10.0, 37); R[5 + 1] = rec(-9.5, 10.0, 10.0, 37); R[5 + 2] = rec(-8.0, 10.0, 10.0, 36);
    R[5 + 3] = rec(1.0, 10.0, 10.0, 900); R[5 + 4] = rec(-9.0, 10.0, 10.0, 38);
    /* port 2: one silent block (no energy), lags {-5, -3}: lower median -5; corr sums to > 0 although one block is negative */
    R[10 + 0] = rec(6.0, 10.0, 10.0, -5); R[10 + 1] = rec(-5.5, 10.0, 10.0, -3); R[10 + 2] = rec(0.0, 0.0, 10.0, 77); R[10 + 3] = rec(5.0, 10.0, 0.0, 78);
    /* port 3: against itself: lag 0 whatever its records say */
    for (int i = 0; i < 5; i++) R[15 + i] = rec(10.0, 10.0, 10.0, 11);
    const int pf[4] = { 0, 3, 5, 6 }, pch[6] = { 0, 1, 2, 2, 1, 3 };
    int delay[6], sign[6];
    for (int i = 0; i < 6; i++) delay[i] = sign[i] = 99;
    CHECK(gdg_blend_plan_delays(R.data(), 4, 5, ref, 0.5, 3, pf, pch, delay, sign, &b) == BLEND_PLAN_OK && b == -1);
    /* blend 0: lags {0, 37, -5} -> delays {37, 0, 42}; blend 1: lags {-5, 37} -> {42, 0}; blend 2: port 3 alone */
    CHECK(delay[0] == 37 && delay[1] == 0 && delay[2] == 42 && sign[0] == 1 && sign[1] == -1 && sign[2] == 1);
    CHECK(delay[3] == 42 && delay[4] == 0 && sign[3] == 1 && sign[4] == -1);
    CHECK(delay[5] == 0 && sign[5] == 1);
    /* a lower threshold lets the weak block in: {36, 37, 37, 38, 900} -> 37 still; a threshold nothing passes: lag 0, sign +1 */
    CHECK(gdg_blend_plan_delays(R.data(), 4, 5, ref, 0.05, 1, pf, pch, delay, sign, &b) == BLEND_PLAN_OK && delay[0] == 37 && delay[1] == 0);
    CHECK(gdg_blend_plan_delays(R.data(), 4, 5, ref, 0.99, 1, pf, pch, delay, sign, &b) == BLEND_PLAN_OK && delay[0] == 0 && delay[1] == 0 && delay[2] == 0 && sign[1] == 1);
    /* an even count: the LOWER median */
    R[5 + 3] = rec(-9.0, 10.0, 10.0, 40);                                     /* port 1: {36, 37, 37, 38, 40} -> 37; drop one 37 below */
    R[5 + 1] = rec(-0.1, 10.0, 10.0, 37);                                     /* weak now: {36, 37, 38, 40} -> 37 */
    CHECK(gdg_blend_plan_delays(R.data(), 4, 5, ref, 0.5, 1, pf, pch, delay, sign, &b) == BLEND_PLAN_OK && delay[0] == 37);
    R[5 + 0] = rec(-9.0, 10.0, 10.0, 39);                                     /* {36, 38, 39, 40} -> 38 */
    CHECK(gdg_blend_plan_delays(R.data(), 4, 5, ref, 0.5, 1, pf, pch, delay, sign, &b) == BLEND_PLAN_OK && delay[0] == 38 && delay[2] == 43);
    /* mixed references: blend 1 of {0 (against nothing), 3 (against itself)}; and of {1 (against 0), 3}: nothing is written */
    const int mf[3] = { 0, 2, 4 }, mch[4] = { 0, 1, 1, 3 }, mch2[4] = { 0, 1, 0, 3 };
    for (int i = 0; i < 6; i++) delay[i] = sign[i] = 99;
    CHECK(gdg_blend_plan_delays(R.data(), 4, 5, ref, 0.5, 2, mf, mch, delay, sign, &b) == BLEND_PLAN_MIXED && b == 1);
    CHECK(gdg_blend_plan_delays(R.data(), 4, 5, ref, 0.5, 2, mf, mch2, delay, sign, &b) == BLEND_PLAN_MIXED && b == 1);
    for (int i = 0; i < 6; i++) CHECK(delay[i] == 99 && sign[i] == 99);
    /* two ports with two different references */
    const int ref2[4] = { -1, 0, 3, -1 };
    const int tf[2] = { 0, 2 }, tch[2] = { 1, 2 };
    CHECK(gdg_blend_plan_delays(R.data(), 4, 5, ref2, 0.5, 1, tf, tch, delay, sign, &b) == BLEND_PLAN_MIXED && b == 0);
    /* both measured against a port that is no term: fine, the reference need not be in the blend */
    const int ref3[4] = { -1, 0, 0, -1 };
    CHECK(gdg_blend_plan_delays(R.data(), 4, 5, ref3, 0.5, 1, tf, tch, delay, sign, &b) == BLEND_PLAN_OK && delay[0] == 0 && delay[1] == 43);
    /* arguments */
    const int bad_ch[2] = { 1, 4 }, bad_f[2] = { 0, 0 };
    CHECK(gdg_blend_plan_delays(R.data(), 4, 5, ref3, 0.5, 1, tf, bad_ch, delay, sign, &b) == BLEND_PLAN_LIST && b == 0);
    CHECK(gdg_blend_plan_delays(R.data(), 4, 5, ref3, 0.5, 1, bad_f, tch, delay, sign, &b) == BLEND_PLAN_LIST && b == 0);
    CHECK(gdg_blend_plan_delays(R.data(), 4, 5, ref3, 1.5, 1, tf, tch, delay, sign, &b) == BLEND_PLAN_ARGS);
    CHECK(gdg_blend_plan_delays(R.data(), 4, 5, ref3, std::numeric_limits<double>::quiet_NaN(), 1, tf, tch, delay, sign, &b) == BLEND_PLAN_ARGS);
    CHECK(gdg_blend_plan_delays(R.data(), 4, 5, nullptr, 0.5, 1, tf, tch, delay, sign, &b) == BLEND_PLAN_ARGS);
    CHECK(gdg_blend_plan_delays(nullptr, 4, 0, ref3, 0.5, 1, tf, tch, delay, sign, &b) == BLEND_PLAN_OK && delay[0] == 0 && delay[1] == 0);      /* no blocks: every lag 0 */
    if (failures) { printf("FAILED %d checks\n", failures); return 1; }
    printf("OK\n");
    return 0;
}
