/* csrc/blend.h on the host, under AddressSanitizer and UBSan (tests/test_blend_filter_host.py): a list set with tap_first == NULL packs the
 * delayed table byte for byte, and so does a list whose every term has no tap; a list with taps packs first | channel | delay | tap_first |
 * weight | gain | taps; every refusal of the taps names blend and term and leaves the list in force as it was; the filtered sum on the host
 * against the known answer of include/gdg.h; the taps of a fractional delay; and the planner that picks the fraction from fit records -- the
 * winner, the tie rule, silent candidates, the refusals; the one table and its view over every list shape, the bytes the batch uploads against a
 * literal, and the plain and delayed host sums as the filtered one with absent arguments.  No device, no context. */
#include "blend.h"
#include <cmath>
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

/* ---- one table, one view (blend.h: gdg_blend_pack, gdg_blend_view_at, BlendSet::pack) ---- */
/* a list of the given term counts with T taps on every term (T < 0: no tap_first), packed with and without each optional part: the view of
 * the bytes points at values equal to the inputs, every double is 8-byte aligned, and the last byte read is the buffer's last */
static void pack_and_view(const std::vector<int> &terms_of, int T, bool with_delay, bool with_gain) {
    const int n_blends = (int)terms_of.size();
    std::vector<int> first(1, 0), channel, delay, tap_first(1, 0);
    std::vector<double> weight, gain, tap;
    for (int b = 0; b < n_blends; b++) {
        for (int k = 0; k < terms_of[(size_t)b]; k++) {
            channel.push_back((b + 3 * k) % 5);
            weight.push_back(0.25 * (double)(k + 1) - (double)b);
            delay.push_back((7 * k + b) % (GDG_BLEND_MAX_DELAY - 64));
            for (int t = 0; t < (T > 0 ? T : 0); t++) tap.push_back(1.0 / (double)(1 + t + k));
            tap_first.push_back((int)tap.size());
        }
        first.push_back((int)channel.size());
        gain.push_back(0.5 + (double)b);
    }
    const int terms = (int)channel.size();
    tap.push_back(9.0);                                                      /* a spare entry: a list without a tap still has an address */
    const std::vector<unsigned char> bytes = gdg_blend_pack(n_blends, first.data(), channel.data(), weight.data(), with_gain ? gain.data() : nullptr,
                                                            with_delay ? delay.data() : nullptr, T >= 0 ? tap_first.data() : nullptr, tap.data());
    size_t size = 0;
    const gdg_blend_view v = gdg_blend_view_at(bytes.data(), n_blends, terms, with_delay, T >= 0 ? tap_first[(size_t)terms] : -1, with_gain, &size);
    CHECK(size == bytes.size() && v.n_blends == n_blends);
    CHECK(v.first && v.channel && v.weight && !memcmp(v.first, first.data(), first.size() * sizeof(int)) && !memcmp(v.channel, channel.data(), channel.size() * sizeof(int)) &&
          !memcmp(v.weight, weight.data(), weight.size() * sizeof(double)));
    CHECK(with_delay ? v.delay && !memcmp(v.delay, delay.data(), delay.size() * sizeof(int)) : !v.delay);
    CHECK(with_gain ? v.gain && !memcmp(v.gain, gain.data(), gain.size() * sizeof(double)) : !v.gain);
    CHECK(T >= 0 ? v.tap_first && v.tap && !memcmp(v.tap_first, tap_first.data(), tap_first.size() * sizeof(int)) && !memcmp(v.tap, tap.data(), (tap.size() - 1) * sizeof(double))
                 : !v.tap_first && !v.tap);
    CHECK((uintptr_t)bytes.data() % 8 == 0 && (uintptr_t)v.weight % 8 == 0 && (uintptr_t)v.gain % 8 == 0 && (uintptr_t)v.tap % 8 == 0);
    /* the last part that is there ends where the buffer ends, and the first begins where it begins */
    const unsigned char *end = T >= 0 ? (const unsigned char *)(v.tap + (tap.size() - 1)) : with_gain ? (const unsigned char *)(v.gain + n_blends) : (const unsigned char *)(v.weight + terms);
    CHECK(end == bytes.data() + bytes.size() && (const unsigned char *)v.first == bytes.data());
}

static void one_table_one_view() {
    const std::vector<std::vector<int>> shapes = { { 1 }, { 32, 1, 5 } };
    for (const std::vector<int> &terms_of : shapes)
        for (int gains = 0; gains < 2; gains++) {
            pack_and_view(terms_of, -1, false, gains);                        /* plain */
            pack_and_view(terms_of, -1, true, gains);                         /* delays only */
            for (int T : { 0, 1, 2, 63, 64 }) {
                pack_and_view(terms_of, T, false, gains);                     /* taps, delays absent */
                pack_and_view(terms_of, T, true, gains);
            }
        }
    size_t size = 9;
    const gdg_blend_view none = gdg_blend_view_at(nullptr, 0, 0, false, -1, false, &size);
    CHECK(size == 0 && !none.first && !none.weight && gdg_blend_pack(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr).empty());
    /* the layout the batch uploads, byte for byte (little-endian): first | channel | delay | tap_first | pad to 8 | weight | gain | taps */
    const int first[3] = { 0, 2, 3 }, channel[3] = { 0, 1, 2 }, delay[3] = { 0, 7, 1 }, tap_first[4] = { 0, 2, 2, 5 };
    const double weight[3] = { 1.0, -1.0, 0.5 }, gain[2] = { 1.0, 2.0 }, tap[5] = { 1.0, -1.0, 0.25, 0.0, -0.5 };
    int b = 0, k = 0;
    BlendSet set;
    CHECK(gdg_blend_replace(set, 2, first, channel, weight, delay, tap_first, tap, gain, 3, &b, &k) == BLEND_OK);
#define I32(v) (v), 0, 0, 0
#define F64(hi, lo) 0, 0, 0, 0, 0, 0, (lo), (hi)
    const unsigned char want[] = { I32(0), I32(2), I32(3), I32(0), I32(1), I32(2), I32(0), I32(7), I32(1), I32(0), I32(2), I32(2), I32(5), 0, 0, 0, 0,
                                   F64(0x3f, 0xf0), F64(0xbf, 0xf0), F64(0x3f, 0xe0),                                    /* 1.0, -1.0, 0.5 */
                                   F64(0x3f, 0xf0), F64(0x40, 0x00),                                                     /* 1.0, 2.0 */
                                   F64(0x3f, 0xf0), F64(0xbf, 0xf0), F64(0x3f, 0xd0), F64(0x00, 0x00), F64(0xbf, 0xe0) };  /* 1.0, -1.0, 0.25, 0.0, -0.5 */
    CHECK(set.packed.size() == sizeof want && !memcmp(set.packed.data(), want, sizeof want));
    /* without taps, and without delays: the same bytes with those parts gone -- 9 ints and 4 bytes of pad, 6 ints */
    CHECK(gdg_blend_replace(set, 2, first, channel, weight, delay, nullptr, nullptr, gain, 3, &b, &k) == BLEND_OK);
    CHECK(set.packed.size() == 40 + 40 && !memcmp(set.packed.data(), want, 36) && !memcmp(set.packed.data() + 40, want + 56, 40));
    CHECK(gdg_blend_replace(set, 2, first, channel, weight, gain, 3, &b, &k) == BLEND_OK);
    CHECK(set.packed.size() == 24 + 40 && !memcmp(set.packed.data(), want, 24) && !memcmp(set.packed.data() + 24, want + 56, 40));
#undef I32
#undef F64
    /* the view of the set is the view of its bytes, wherever they lie */
    CHECK(gdg_blend_replace(set, 2, first, channel, weight, delay, tap_first, tap, gain, 3, &b, &k) == BLEND_OK);
    const gdg_blend_view v = set.view(set.packed.data());
    CHECK(v.n_blends == 2 && v.delay[1] == 7 && v.tap_first[3] == 5 && v.weight[2] == 0.5 && v.gain[1] == 2.0 && v.tap[4] == -0.5);
}

/* ---- one host definition: the plain and the delayed names are the filtered sum with the absent arguments null, bit for bit ---- */
static void one_host_definition() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const size_t samples = 257;
    std::vector<std::vector<double>> x(3, std::vector<double>(samples)), hist(3, std::vector<double>((size_t)GDG_BLEND_MAX_DELAY));
    uint64_t state = 88172645463325252ull;
    auto next = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (double)(int64_t)(state >> 11) / 4503599627370496.0 - 1.0; };
    for (int r = 0; r < 3; r++) {
        for (double &v : x[(size_t)r]) v = next();
        for (double &v : hist[(size_t)r]) v = next();
    }
    x[0][5] = inf; x[1][9] = -inf; x[2][11] = nan; x[0][13] = -0.0; x[1][13] = -0.0; x[2][200] = inf;      /* row 2 carries the zero weight */
    hist[1][(size_t)GDG_BLEND_MAX_DELAY - 1] = inf; hist[2][(size_t)GDG_BLEND_MAX_DELAY - 2] = nan;
    const double *rows[3] = { x[0].data(), x[1].data(), x[2].data() }, *hs[3] = { hist[0].data(), hist[1].data(), hist[2].data() };
    const int first[3] = { 0, 5, 6 }, channel[6] = { 0, 1, 2, 1, 0, 2 }, delay[6] = { 0, 1, 3, 256, 2, 0 };
    const double weight[6] = { 0.75, -1.25, 0.0, 1e-3, -0.0, 1.0 };
    std::vector<double> a(2 * samples), c(2 * samples);
    double *oa[2] = { a.data(), a.data() + samples }, *oc[2] = { c.data(), c.data() + samples };
    gdg_blend_sum_host(rows, samples, 2, first, channel, weight, oa);
    gdg_blend_sum_host_filtered(rows, nullptr, samples, 2, first, channel, weight, nullptr, nullptr, nullptr, oc);
    CHECK(!memcmp(a.data(), c.data(), a.size() * sizeof(double)));
    CHECK(std::isnan(a[200]) && std::isnan(a[5]) && std::isinf(a[samples + 200]));      /* 0.0 * inf; inf + -0.0 * inf; 1.0 * inf */
    for (const double *const *h : { (const double *const *)nullptr, (const double *const *)hs })
        for (const int *d : { (const int *)delay, (const int *)nullptr }) {
            gdg_blend_sum_host_delayed(rows, h, samples, 2, first, channel, weight, d, oa);
            gdg_blend_sum_host_filtered(rows, h, samples, 2, first, channel, weight, d, nullptr, nullptr, oc);
            CHECK(!memcmp(a.data(), c.data(), a.size() * sizeof(double)));
        }
    for (size_t i = 0; i < samples; i += 50)
        CHECK(gdg_blend_sample(rows, i, channel, weight, 0, 5) == gdg_blend_sample_delayed(rows, hs, i, channel, weight, nullptr, 0, 5) || std::isnan(gdg_blend_sample(rows, i, channel, weight, 0, 5)));
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
    one_table_one_view();
    one_host_definition();
    if (failures) { printf("FAILED %d checks\n", failures); return 1; }
    printf("OK\n");
    return 0;
}
