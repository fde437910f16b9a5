/*
 * tapfit_plan_check.cpp -- the tap fit's host arithmetic without HIP: the planner of csrc/blend.h (gdg_blend_plan_taps) against hand-made
 * records whose answers are known in closed form, its bits against the fit planner's for up to 8 unknowns, the list's validation
 * (gdg_tapfit_check, gdg_tapfit_table), and the place and room of the tap-fit section in a step's download half (csrc/report_sections.h).
 * Built by tests/test_tapfit_host.py, once more under AddressSanitizer and UBSan.
 */
#include "blend.h"
#include "report_sections.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

/* the record of integer rows, exactly: virtual row (j, a) = x[p_j][i - a], the target x[t][i], i = T - 1 + n, n = 0 .. L - T */
static std::vector<double> record_of(const std::vector<std::vector<long>> &x, int t, const std::vector<int> &p, int T) {
    const int K = (int)p.size(), U = K * T, V = U + 1, L = (int)x[0].size();
    std::vector<double> rec((size_t)V * (V + 1) / 2, 0.0);
    auto at = [&](int v, int n) { return v < U ? x[(size_t)p[(size_t)(v / T)]][(size_t)(T - 1 + n - v % T)] : x[(size_t)t][(size_t)(T - 1 + n)]; };
    for (int u = 0; u < V; u++)
        for (int v = 0; v <= u; v++) {
            long s = 0;
            for (int n = 0; n + T <= L; n++) s += at(u, n) * at(v, n);
            rec[gdg_gram_index((size_t)u, (size_t)v)] = (double)s;
        }
    return rec;
}

int main() {
    const double untouched = -7.25;
    int fit = 0, row = 0;
    /* U = 1, A = 4, b = 2: h = 0.5, and (Tt - 2 h b + h A h) / Tt = (3 - 2 + 1) / 3 */
    {
        const int first[2] = { 0, 1 }, taps[1] = { 1 };
        const double rec[3] = { 4.0, 2.0, 3.0 };
        double h[2] = { untouched, untouched }, res[2] = { untouched, untouched };
        CHECK(gdg_blend_plan_taps(rec, 1, first, taps, 1, 0.0, h, res, &fit, &row) == TAPS_PLAN_OK && fit == -1 && row == -1);
        CHECK(h[0] == 0.5 && h[1] == untouched && fabs(res[0] - 2.0 / 3.0) <= 1e-15 && res[1] == untouched);
    }
    /* the target is an integer row filtered by the integer taps {1, -2, 3}: every sum is exact.  The row is four impulses of +-2 more than
     * T apart and away from the ends, so A = 16 I: the factor is 4 I, every root and quotient is exact, the taps come back to the last bit
     * and nothing is left; the same over two blocks whose records are added */
    {
        const int L = 40, T = 3;
        std::vector<std::vector<long>> x(2, std::vector<long>((size_t)L, 0));
        x[0][5] = 2; x[0][12] = -2; x[0][20] = 2; x[0][31] = 2;
        const long taps_true[3] = { 1, -2, 3 };
        for (int i = 0; i < L; i++) for (int a = 0; a < T && a <= i; a++) x[1][(size_t)i] += taps_true[a] * x[0][(size_t)(i - a)];
        const int first[2] = { 0, 1 }, taps[1] = { T };
        const std::vector<double> rec = record_of(x, 1, { 0 }, T);
        CHECK(rec.size() == gdg_tapfit_fit_doubles(1, T) && rec.size() == 10);
        double h[3], res[1];
        CHECK(gdg_blend_plan_taps(rec.data(), 1, first, taps, 1, 0.0, h, res, &fit, &row) == TAPS_PLAN_OK);
        CHECK(h[0] == 1.0 && h[1] == -2.0 && h[2] == 3.0 && res[0] == 0.0);
        std::vector<std::vector<long>> x2(2, std::vector<long>((size_t)L, 0));          /* two impulses: A = 8 I per block, 16 I over two */
        x2[0][5] = 2; x2[0][20] = -2;
        for (int i = 0; i < L; i++) for (int a = 0; a < T && a <= i; a++) x2[1][(size_t)i] += taps_true[a] * x2[0][(size_t)(i - a)];
        const std::vector<double> half = record_of(x2, 1, { 0 }, T);
        std::vector<double> two(half);
        two.insert(two.end(), half.begin(), half.end());
        CHECK(gdg_blend_plan_taps(two.data(), 1, first, taps, 2, 0.0, h, res, &fit, &row) == TAPS_PLAN_OK);
        CHECK(h[0] == 1.0 && h[1] == -2.0 && h[2] == 3.0 && res[0] == 0.0);
        /* one port twice: refused with ridge = 0, fit, term and lag named, nothing written; equal taps with a ridge */
        const int first2[3] = { 0, 1, 3 }, taps2[2] = { T, 2 };
        std::vector<double> both(rec);
        const std::vector<double> twice = record_of(x, 1, { 0, 0 }, 2);
        both.insert(both.end(), twice.begin(), twice.end());
        CHECK(gdg_tapfit_list_doubles(2, first2, taps2) == both.size());
        double h5[7], res2[2];
        for (double &v : h5) v = untouched;
        res2[0] = res2[1] = untouched;
        CHECK(gdg_blend_plan_taps(both.data(), 2, first2, taps2, 1, 0.0, h5, res2, &fit, &row) == TAPS_PLAN_PIVOT && fit == 1 && row == 2);      /* term 1, lag 0 */
        for (double v : h5) CHECK(v == untouched);
        CHECK(res2[0] == untouched && res2[1] == untouched);
        /* ... the difference of the two copies' taps lies along the direction the ridge alone holds: roundings of U * 2^-52 grow by 1 / ridge */
        CHECK(gdg_blend_plan_taps(both.data(), 2, first2, taps2, 1, 1e-3, h5, res2, &fit, &row) == TAPS_PLAN_OK && fit == -1);
        const double tol = 4.0 * 2.220446049250313e-16 / 1e-3 * fmax(fabs(h5[3]), fabs(h5[4]));
        CHECK(fabs(h5[3] - h5[5]) <= tol && fabs(h5[4] - h5[6]) <= tol && h5[3] != 0.0 && h5[4] != 0.0);
        /* a NaN entry is refused and named */
        both[gdg_gram_index(1, 0)] = NAN;
        CHECK(gdg_blend_plan_taps(both.data(), 2, first2, taps2, 1, 0.0, h5, res2, &fit, &row) == TAPS_PLAN_NONFINITE && fit == 0 && row == 1);
    }
    /* U <= 8: bit for bit the fit planner's weights for a record holding the same sums, with and without a ridge */
    for (int U = 1; U <= 8; U++)
        for (int T = 1; T <= U; T++) {
            if (U % T) continue;
            const int K = U / T;
            if (K > GDG_TAPFIT_MAX_TERMS) continue;
            unsigned seed = 99u + (unsigned)U * 17u + (unsigned)T;
            auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (double)(seed >> 8) / 16777216.0 - 0.5; };
            /* a positive definite Gram of U + 1 random rows of 24 values */
            std::vector<std::vector<double>> v((size_t)U + 1, std::vector<double>(24));
            for (auto &r : v) for (double &e : r) e = rnd();
            std::vector<double> rec(gdg_tapfit_fit_doubles(K, T));
            gdg_blend_fit_rec fr;
            memset(&fr, 0, sizeof fr);
            fr.terms = (uint32_t)U;
            for (int i = 0; i <= U; i++)
                for (int j = 0; j <= i; j++) {
                    double s = 0.0;
                    for (int n = 0; n < 24; n++) s += v[(size_t)i][(size_t)n] * v[(size_t)j][(size_t)n];
                    rec[gdg_gram_index((size_t)i, (size_t)j)] = s;
                    if (i < U) fr.xx[i * (i + 1) / 2 + j] = s;
                    else if (j < U) fr.tx[j] = s;
                    else fr.tt = s;
                }
            const int first[2] = { 0, K }, taps[1] = { T };
            for (double ridge : { 0.0, 0.01 }) {
                double h[8], res[1], w[8], wres[1];
                int bad = 0;
                CHECK(gdg_blend_plan_taps(rec.data(), 1, first, taps, 1, ridge, h, res, &fit, &row) == TAPS_PLAN_OK);
                CHECK(gdg_blend_plan_weights(&fr, 1, 1, ridge, w, wres, &bad) == FIT_PLAN_OK);
                CHECK(memcmp(h, w, (size_t)U * sizeof(double)) == 0 && memcmp(res, wres, sizeof(double)) == 0);
            }
        }
    /* the list: every refusal names its fit and term */
    {
        int term = 0;
        const int first[3] = { 0, 2, 3 }, port[3] = { 0, 1, 2 }, target[2] = { 3, 0 }, taps[2] = { 64, 5 };
        CHECK(gdg_tapfit_check(2, first, port, target, taps, 4, &fit, &term) == TAPFIT_OK && fit == -1 && term == -1);
        CHECK(gdg_tapfit_check(2, first, port, target, taps, -1, &fit, &term) == TAPFIT_OK);
        CHECK(gdg_tapfit_check(2, first, port, target, taps, 3, &fit, &term) == TAPFIT_TARGET && fit == 0 && term == -1);
        CHECK(gdg_tapfit_check(2, first, port, target, taps, 2, &fit, &term) == TAPFIT_TARGET && fit == 0);
        const int target_ok[2] = { 0, 0 };
        CHECK(gdg_tapfit_check(2, first, port, target_ok, taps, 2, &fit, &term) == TAPFIT_PORT && fit == 1 && term == 0);
        CHECK(gdg_tapfit_check(17, first, port, target, taps, 4, &fit, &term) == TAPFIT_COUNT && gdg_tapfit_check(-1, first, port, target, taps, 4, &fit, &term) == TAPFIT_COUNT);
        CHECK(gdg_tapfit_check(0, nullptr, nullptr, nullptr, nullptr, 4, &fit, &term) == TAPFIT_OK);
        CHECK(gdg_tapfit_check(2, first, port, target, nullptr, 4, &fit, &term) == TAPFIT_NULL);
        const int first_bad[3] = { 1, 2, 3 }, first_desc[3] = { 0, 2, 1 }, first_none[3] = { 0, 2, 2 }, first_five[2] = { 0, 5 }, first_three[2] = { 0, 3 };
        CHECK(gdg_tapfit_check(2, first_bad, port, target, taps, 4, &fit, &term) == TAPFIT_FIRST && fit == 0);
        CHECK(gdg_tapfit_check(2, first_desc, port, target, taps, 4, &fit, &term) == TAPFIT_FIRST && fit == 1);
        CHECK(gdg_tapfit_check(2, first_none, port, target, taps, 4, &fit, &term) == TAPFIT_TERMS && fit == 1);
        const int port5[5] = { 0, 1, 2, 3, 0 }, taps_two[1] = { 2 }, taps_0[2] = { 64, 0 }, taps_65[2] = { 65, 5 }, taps_64[1] = { 64 };
        CHECK(gdg_tapfit_check(1, first_five, port5, target, taps_two, 4, &fit, &term) == TAPFIT_TERMS && fit == 0);
        CHECK(gdg_tapfit_check(2, first, port, target, taps_0, 4, &fit, &term) == TAPFIT_TAPS && fit == 1);
        CHECK(gdg_tapfit_check(2, first, port, target, taps_65, 4, &fit, &term) == TAPFIT_TAPS && fit == 0);
        CHECK(gdg_tapfit_check(1, first_three, port5, target, taps_64, 4, &fit, &term) == TAPFIT_UNKNOWNS && fit == 0);
        /* the table: offsets and tiles run on from fit to fit */
        const std::vector<int> t = gdg_tapfit_table(2, first, port, target, taps);
        CHECK(t.size() == 2 * GDG_TAPFIT_TABLE_INTS && GDG_TAPFIT_TABLE_INTS == 9);
        CHECK(t[TAPFIT_E_TARGET] == 3 && t[TAPFIT_E_TERMS] == 2 && t[TAPFIT_E_TAPS] == 64 && t[TAPFIT_E_PORT] == 0 && t[TAPFIT_E_PORT + 1] == 1 && t[TAPFIT_E_OFFSET] == 0 && t[TAPFIT_E_TILE0] == 0);
        const int *e = &t[GDG_TAPFIT_TABLE_INTS];
        CHECK(e[TAPFIT_E_TARGET] == 0 && e[TAPFIT_E_TERMS] == 1 && e[TAPFIT_E_TAPS] == 5 && e[TAPFIT_E_PORT] == 2 && e[TAPFIT_E_OFFSET] == 129 * 130 / 2 && e[TAPFIT_E_TILE0] == 15);
        CHECK(gdg_tapfit_list_doubles(2, first, taps) == 129 * 130 / 2 + 6 * 7 / 2);
        TapFitSet set;
        set.table = t;
        CHECK(set.count() == 2 && set.doubles() == 129 * 130 / 2 + 21 && set.first_outside(4, &term) == -1 && set.first_outside(3, &term) == 0 && term == -1);
        CHECK(set.first_outside(2, &term) == 0 && set.first_outside(1, &term) == 0);
    }
    /* the section: behind `end` from the next 16 bytes on, [w] records of D doubles; nothing for no fit */
    int cases = 0, moved = 0;
    for (size_t end : { (size_t)0, (size_t)8, (size_t)16, (size_t)1000, (size_t)4097 })
        for (size_t D : { (size_t)0, (size_t)3, (size_t)2145, (size_t)134160 })
            for (size_t w : { (size_t)1, (size_t)2, (size_t)16 }) {
                const ListShape shape = { 1, D * 8 };
                const ListSection s = list_section(end, shape, w);
                cases++;
                if (!D) { CHECK(s.at == end && s.bytes == 0 && s.end == end && list_room(shape, w) == 0); continue; }
                CHECK(s.at % 16 == 0 && s.at >= end && s.at < end + 16 && s.bytes == w * D * 8 && s.end == s.at + s.bytes);
                CHECK(s.end - end <= list_room(shape, w) && list_room(shape, w) == 16 + w * D * 8);
                moved += s.at != end;
            }
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("OK tap-fit planner, list and section; %d section cases, %d moved by the 16-byte step\n", cases, moved);
    return 0;
}
