/* csrc/blend.h on the host, under AddressSanitizer and UBSan (tests/test_blend_filter_host.py): a list set with tap_first == NULL packs the
 * delayed table byte for byte, and so does a list whose every term has no tap; a list with taps packs first | channel | delay | tap_first |
 * weight | gain | taps; every refusal of the taps names blend and term and leaves the list in force as it was; the filtered sum on the host
 * against the known answer of include/gdg.h; the taps of a fractional delay; and the planner that picks the fraction from fit records -- the
 * winner, the tie rule, silent candidates, the refusals.  No device, no context. */
#include "blend.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

/* one fit's record of K candidates: tt, tx[k], and xx[k][k] on the diagonal */
static gdg_blend_fit_rec fit_rec(int K, double tt, const double *tx, const double *xx) {
    gdg_blend_fit_rec r;
    memset(&r, 0, sizeof r);
    r.tt = tt;
    r.terms = (uint32_t)K;
    for (int k = 0; k < K; k++) { r.tx[k] = tx[k]; r.xx[k * (k + 1) / 2 + k] = xx[k]; }
    return r;
}

int main() {
    int b = 0, k = 0, t = 0;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    /* ---- tap_first == NULL is the delayed list, byte for byte; so is a list whose every T is 0 ---- */
    const int f_ok[3] = { 0, 2, 3 }, ch_ok[3] = { 0, 1, 2 }, d_ok[3] = { 0, 7, 1 }, d_zero[3] = { 0, 0, 0 };
    const double w_ok[3] = { 0.6, 0.4, -1.0 }, g_ok[2] = { 1.0, 0.5 };
    for (const int *d : { (const int *)d_ok, (const int *)d_zero, (const int *)nullptr }) {
        BlendSet delayed, null_taps, no_taps;
        const int tf0[4] = { 0, 0, 0, 0 };
        const double spare[1] = { 0.0 };
        CHECK(gdg_blend_replace(delayed, 2, f_ok, ch_ok, w_ok, d, g_ok, 3, &b, &k) == BLEND_OK);
        CHECK(gdg_blend_replace(null_taps, 2, f_ok, ch_ok, w_ok, d, (const int *)nullptr, (const double *)nullptr, g_ok, 3, &b, &k) == BLEND_OK);
        CHECK(gdg_blend_replace(no_taps, 2, f_ok, ch_ok, w_ok, d, tf0, spare, g_ok, 3, &b, &k) == BLEND_OK);
        CHECK(!delayed.packed.empty() && null_taps.packed == delayed.packed && no_taps.packed == delayed.packed);
        CHECK(null_taps.tap_first.empty() && null_taps.tap.empty() && no_taps.tap_first.empty() && no_taps.delay == delayed.delay);
        CHECK(null_taps.max_reach() == delayed.max_delay() && no_taps.max_reach() == delayed.max_delay() && null_taps.packed_ints() == delayed.packed_ints());
    }
    /* ---- a list with taps: T = {2, 0, 3}, d = {0, 7, 1} ---- */
    const int tf_ok[4] = { 0, 2, 2, 5 };
    const double h_ok[5] = { 1.0, -1.0, 0.25, 0.0, -0.5 };
    BlendSet set;
    CHECK(gdg_blend_replace(set, 2, f_ok, ch_ok, w_ok, d_ok, tf_ok, h_ok, g_ok, 3, &b, &k) == BLEND_OK && b == -1 && k == -1);
    CHECK(set.taps(0) == 2 && set.taps(1) == 0 && set.taps(2) == 3 && set.max_delay() == 7 && set.max_reach() == 7);
    /* 3 + 3 + 3 + 4 ints = 52 bytes, padded to 56; 3 weights, 2 gains, 5 taps */
    CHECK(set.packed_ints() == 56 && set.packed_taps() == 56 + 5 * sizeof(double) && set.packed.size() == 56 + 10 * sizeof(double));
    { int v[4]; memcpy(v, set.packed.data() + 9 * sizeof(int), sizeof v); CHECK(v[0] == 0 && v[1] == 2 && v[2] == 2 && v[3] == 5); }
    { int v[3]; memcpy(v, set.packed.data() + 6 * sizeof(int), sizeof v); CHECK(v[0] == 0 && v[1] == 7 && v[2] == 1); }
    { double v[5]; memcpy(v, set.packed.data() + set.packed_taps(), sizeof v); CHECK(v[0] == 1.0 && v[1] == -1.0 && v[2] == 0.25 && v[3] == 0.0 && v[4] == -0.5); }
    { double v[2]; memcpy(v, set.packed.data() + 56 + 3 * sizeof(double), sizeof v); CHECK(v[0] == 1.0 && v[1] == 0.5); }
    /* taps and no delay list: the delays are there as zeros; a reach of T - 1 */
    BlendSet only_taps;
    CHECK(gdg_blend_replace(only_taps, 2, f_ok, ch_ok, w_ok, (const int *)nullptr, tf_ok, h_ok, nullptr, 3, &b, &k) == BLEND_OK);
    CHECK(only_taps.delay.size() == 3 && only_taps.max_delay() == 0 && only_taps.max_reach() == 2);
    /* T = 1 and d = 0: a filtered list that reaches nowhere */
    const int tf_one[4] = { 0, 1, 1, 1 };
    BlendSet one;
    CHECK(gdg_blend_replace(one, 2, f_ok, ch_ok, w_ok, (const int *)nullptr, tf_one, h_ok, nullptr, 3, &b, &k) == BLEND_OK && one.max_reach() == 0 && !one.tap_first.empty());

    /* ---- the refusals: blend and term named, the list in force unchanged ---- */
    const BlendSet kept = set;
    auto unchanged = [&]() { return set.packed == kept.packed && set.tap == kept.tap && set.tap_first == kept.tap_first && set.delay == kept.delay && set.weight == kept.weight; };
    const double h_nan[5] = { 1.0, -1.0, 0.25, nan, -0.5 }, h_inf[5] = { 1.0, inf, 0.25, 0.0, -0.5 };
    CHECK(gdg_blend_replace(set, 2, f_ok, ch_ok, w_ok, d_ok, tf_ok, h_nan, g_ok, 3, &b, &k) == BLEND_TAP && b == 1 && k == 0 && unchanged());
    CHECK(gdg_blend_check_taps(2, f_ok, d_ok, tf_ok, h_nan, &b, &k, &t) == BLEND_TAP && b == 1 && k == 0 && t == 1);
    CHECK(gdg_blend_replace(set, 2, f_ok, ch_ok, w_ok, d_ok, tf_ok, h_inf, g_ok, 3, &b, &k) == BLEND_TAP && b == 0 && k == 0 && unchanged());
    std::vector<double> many(70, 0.5);
    const int tf_65[4] = { 0, 2, 67, 70 }, tf_64[4] = { 0, 2, 66, 70 };
    CHECK(gdg_blend_replace(set, 2, f_ok, ch_ok, w_ok, d_ok, tf_65, many.data(), g_ok, 3, &b, &k) == BLEND_TAP_COUNT && b == 0 && k == 1 && unchanged());
    CHECK(gdg_blend_check_taps(2, f_ok, d_ok, tf_64, many.data(), &b, &k, &t) == BLEND_OK && b == -1 && k == -1);
    const int tf_down[4] = { 0, 2, 1, 5 }, tf_start[4] = { 1, 2, 2, 5 };
    CHECK(gdg_blend_replace(set, 2, f_ok, ch_ok, w_ok, d_ok, tf_down, h_ok, g_ok, 3, &b, &k) == BLEND_TAP_FIRST && b == 0 && k == 1 && unchanged());
    CHECK(gdg_blend_replace(set, 2, f_ok, ch_ok, w_ok, d_ok, tf_start, h_ok, g_ok, 3, &b, &k) == BLEND_TAP_FIRST && b == 0 && k == 0 && unchanged());
    /* the reach: d + T - 1 = 4096 passes, 4097 does not; T = 0 and T = 1 reach d */
    const int d_far[3] = { 0, GDG_BLEND_MAX_DELAY, GDG_BLEND_MAX_DELAY - 2 }, d_over[3] = { 0, GDG_BLEND_MAX_DELAY, GDG_BLEND_MAX_DELAY - 1 };
    CHECK(gdg_blend_check_taps(2, f_ok, d_far, tf_ok, h_ok, &b, &k, &t) == BLEND_OK);
    CHECK(gdg_blend_replace(set, 2, f_ok, ch_ok, w_ok, d_over, tf_ok, h_ok, g_ok, 3, &b, &k) == BLEND_REACH && b == 1 && k == 0 && unchanged());
    const int d_one[3] = { GDG_BLEND_MAX_DELAY, 0, 0 };
    CHECK(gdg_blend_check_taps(2, f_ok, d_one, tf_one, h_ok, &b, &k, &t) == BLEND_OK);
    CHECK(gdg_blend_check_taps(2, f_ok, d_one, tf_ok, h_ok, &b, &k, &t) == BLEND_REACH && b == 0 && k == 0);
    /* what the delayed check refuses comes first, and taps without a tap list are refused */
    const int d_neg[3] = { 0, -1, 0 };
    CHECK(gdg_blend_replace(set, 2, f_ok, ch_ok, w_ok, d_neg, tf_ok, h_nan, g_ok, 3, &b, &k) == BLEND_DELAY && b == 0 && k == 1 && unchanged());
    CHECK(gdg_blend_replace(set, 2, f_ok, ch_ok, w_ok, d_ok, tf_ok, (const double *)nullptr, g_ok, 3, &b, &k) == BLEND_NULL && unchanged());

    /* ---- the known answer: one term, d = 0, T = 2, h = {1, -1}, w = 1: the first difference, the bits of the DELAYS known answer ---- */
    const double x[6] = { 0.5, -0.25, 3.0, 3.0, -0.0, 1e-300 };
    const double *rows1[1] = { x };
    const int ff[2] = { 0, 1 }, fch[1] = { 0 }, fd[1] = { 0 }, ftf[2] = { 0, 2 };
    const double fw[1] = { 1.0 }, fh[2] = { 1.0, -1.0 };
    double o[6], o2[6];
    double *out1[1] = { o }, *out2[1] = { o2 };
    gdg_blend_sum_host_filtered(rows1, nullptr, 6, 1, ff, fch, fw, fd, ftf, fh, out1);
    CHECK(o[0] == 0.5 && o[1] == -0.75 && o[2] == 3.25 && o[3] == 0.0 && o[4] == -3.0 && o[5] == 1e-300);
    const int df[2] = { 0, 2 }, dch[2] = { 0, 0 }, dd[2] = { 0, 1 };
    const double dw[2] = { 1.0, -1.0 };
    gdg_blend_sum_host_delayed(rows1, nullptr, 6, 1, df, dch, dw, dd, out2);
    CHECK(memcmp(o, o2, sizeof o) == 0);
    /* with a history, d = 4095 and two taps: the oldest samples of the run */
    std::vector<double> hist((size_t)GDG_BLEND_MAX_DELAY, 7.0);
    hist[(size_t)GDG_BLEND_MAX_DELAY - 1] = 2.0;
    hist[0] = -4.0;
    const double *h1[1] = { hist.data() };
    gdg_blend_sum_host_filtered(rows1, h1, 6, 1, ff, fch, fw, fd, ftf, fh, out1);
    CHECK(o[0] == -1.5 && o[1] == -0.75);
    const int fd_far[1] = { GDG_BLEND_MAX_DELAY - 1 };
    gdg_blend_sum_host_filtered(rows1, h1, 6, 1, ff, fch, fw, fd_far, ftf, fh, out1);
    CHECK(o[0] == 7.0 - -4.0 && o[1] == 0.0 && o[5] == 0.0);                  /* x[-4095] - x[-4096], then 7 - 7 */
    /* no taps anywhere: the delayed sum */
    gdg_blend_sum_host_filtered(rows1, h1, 6, 1, df, dch, dw, dd, nullptr, nullptr, out1);
    gdg_blend_sum_host_delayed(rows1, h1, 6, 1, df, dch, dw, dd, out2);
    CHECK(memcmp(o, o2, sizeof o) == 0);

    /* ---- the taps of a fractional delay ---- */
    for (int T : { 2, 24, 64 }) {
        double h[GDG_BLEND_MAX_TAPS];
        for (double &v : h) v = 9.0;
        CHECK(gdg_blend_fraction_taps_plan(T, 0.0, h));
        for (int i = 0; i < T; i++) CHECK(h[i] == (i == T / 2 - 1 ? 1.0 : 0.0) && !std::signbit(h[i]));
        for (double f : { 0.25, 0.5, 0.999 }) {
            CHECK(gdg_blend_fraction_taps_plan(T, f, h));
            double sum = 0.0, most = 0.0;
            int at = -1;
            for (int i = 0; i < T; i++) { sum += h[i]; if (fabs(h[i]) > most) { most = fabs(h[i]); at = i; } }
            CHECK(fabs(sum - 1.0) <= (double)(T + 2) * 2.220446049250313e-16);      /* T quotients of half an ulp each, T - 1 adds */
            CHECK(at == (f < 0.5 ? T / 2 - 1 : f > 0.5 ? T / 2 : at) && (at == T / 2 - 1 || at == T / 2));
        }
    }
    { double h2[2]; CHECK(gdg_blend_fraction_taps_plan(2, 0.5, h2) && h2[0] == h2[1] && h2[0] == 0.5); }
    {
        double h[GDG_BLEND_MAX_TAPS + 2];
        for (double &v : h) v = 9.0;
        CHECK(!gdg_blend_fraction_taps_plan(3, 0.5, h) && !gdg_blend_fraction_taps_plan(0, 0.5, h) && !gdg_blend_fraction_taps_plan(66, 0.5, h));
        CHECK(!gdg_blend_fraction_taps_plan(8, 1.0, h) && !gdg_blend_fraction_taps_plan(8, -0.1, h) && !gdg_blend_fraction_taps_plan(8, nan, h));
        CHECK(!gdg_blend_fraction_taps_plan(8, 0.5, nullptr));
        for (double v : h) CHECK(v == 9.0);
    }

    /* ---- the fraction from fit records ---- */
    {
        /* Q = 2: three candidates at -1/2, 0, +1/2; two fits of two blocks */
        const double tx_a0[3] = { 1.0, 2.0, 4.0 }, tx_a1[3] = { 1.0, 2.0, 4.0 }, xx_a[3] = { 2.0, 2.0, 8.0 };      /* scores 1, 2, 2: the tie goes to the earlier */
        const double tx_b0[3] = { 5.0, 9.0, -1.0 }, tx_b1[3] = { 5.0, -8.5, -1.0 }, xx_b[3] = { 2.0, 0.0, 0.5 };     /* the middle one is silent; 10 / 2 against -2 / 1 */
        std::vector<gdg_blend_fit_rec> R = { fit_rec(3, 1.0, tx_a0, xx_a), fit_rec(3, 1.0, tx_a1, xx_a), fit_rec(3, 1.0, tx_b0, xx_b), fit_rec(3, 1.0, tx_b1, xx_b) };
        int step[2] = { 9, 9 };
        CHECK(gdg_blend_plan_fractions(R.data(), 2, 2, 2, step, &b) == FRACTION_OK && b == -1 && step[0] == 0 && step[1] == -1);
        /* the later candidate has to be LARGER to win */
        R[1].tx[2] = 4.5;
        CHECK(gdg_blend_plan_fractions(R.data(), 2, 2, 2, step, &b) == FRACTION_OK && step[0] == 1);
        /* every candidate negative: the largest still wins; all silent or a silent target: 0 */
        const double tx_n[3] = { -3.0, -1.0, -2.0 }, xx_1[3] = { 1.0, 1.0, 1.0 }, xx_0[3] = { 0.0, 0.0, 0.0 };
        std::vector<gdg_blend_fit_rec> N = { fit_rec(3, 1.0, tx_n, xx_1), fit_rec(3, 1.0, tx_n, xx_0), fit_rec(3, 0.0, tx_a0, xx_a) };
        int s3[3] = { 9, 9, 9 };
        CHECK(gdg_blend_plan_fractions(N.data(), 3, 1, 2, s3, &b) == FRACTION_OK && s3[0] == 0 && s3[1] == 0 && s3[2] == 0);
        N[0].tx[0] = -0.5;
        CHECK(gdg_blend_plan_fractions(N.data(), 3, 1, 2, s3, &b) == FRACTION_OK && s3[0] == -1);
        /* Q = 1: one candidate, always 0; Q = 4: seven, the last at +3 */
        const double tx_7[7] = { 0, 1, 2, 3, 4, 5, 6.5 }, xx_7[7] = { 1, 1, 1, 1, 1, 1, 1 };
        gdg_blend_fit_rec r1 = fit_rec(1, 1.0, tx_a0, xx_a), r7 = fit_rec(7, 2.0, tx_7, xx_7);
        int s1 = 9;
        CHECK(gdg_blend_plan_fractions(&r1, 1, 1, 1, &s1, &b) == FRACTION_OK && s1 == 0);
        CHECK(gdg_blend_plan_fractions(&r7, 1, 1, 4, &s1, &b) == FRACTION_OK && s1 == 3);
        /* refusals: nothing is written */
        step[0] = step[1] = 9;
        CHECK(gdg_blend_plan_fractions(R.data(), 2, 2, 3, step, &b) == FRACTION_TERMS && b == 0);
        R[3].terms = 2;
        CHECK(gdg_blend_plan_fractions(R.data(), 2, 2, 2, step, &b) == FRACTION_TERMS && b == 1);
        R[3].terms = 3;
        R[2].tx[0] = inf;
        CHECK(gdg_blend_plan_fractions(R.data(), 2, 2, 2, step, &b) == FRACTION_NONFINITE && b == 1);
        R[2].tx[0] = 5.0;
        R[3].tt = nan;
        CHECK(gdg_blend_plan_fractions(R.data(), 2, 2, 2, step, &b) == FRACTION_NONFINITE && b == 1);
        R[3].tt = 1.0;
        R[3].xx[5] = inf;                                                    /* xx[2][2] */
        CHECK(gdg_blend_plan_fractions(R.data(), 2, 2, 2, step, &b) == FRACTION_NONFINITE && b == 1);
        R[3].xx[5] = 0.5;
        CHECK(gdg_blend_plan_fractions(R.data(), 2, 2, 0, step, &b) == FRACTION_ARGS && gdg_blend_plan_fractions(R.data(), 2, 2, 5, step, &b) == FRACTION_ARGS);
        CHECK(gdg_blend_plan_fractions(R.data(), 2, 0, 2, step, &b) == FRACTION_ARGS && gdg_blend_plan_fractions(nullptr, 2, 2, 2, step, &b) == FRACTION_ARGS);
        CHECK(gdg_blend_plan_fractions(R.data(), 2, 2, 2, nullptr, &b) == FRACTION_ARGS && gdg_blend_plan_fractions(R.data(), -1, 2, 2, step, &b) == FRACTION_ARGS);
        CHECK(step[0] == 9 && step[1] == 9);
        CHECK(gdg_blend_plan_fractions(nullptr, 0, 0, 2, nullptr, &b) == FRACTION_OK);
    }
    if (failures) { printf("FAILED %d checks\n", failures); return 1; }
    printf("OK\n");
    return 0;
}
