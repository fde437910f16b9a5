/*
 * gram_plan_check.cpp -- the Gram list's host arithmetic without HIP: the place and room of the Gram section in a step's download half
 * (csrc/report_sections.h: list_section, list_room with the Gram list's shape) against the formula spelled out here; the packed index of a record (csrc/blend.h:
 * gdg_gram_index) against a full matrix; the list's checks; and the greedy planner (gdg_blend_pick) on hand-made Grams whose answers are
 * known, its weights against the fit planner's on a fit record with the same sums.  Built by tests/test_gram_host.py, once more under
 * AddressSanitizer and UBSan.
 */
#include "blend.h"
#include "report_sections.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

/* the packed record of a full symmetric matrix */
static std::vector<double> pack(const std::vector<double> &full, int P) {
    std::vector<double> r(gdg_gram_doubles((size_t)P));
    for (int i = 0; i < P; i++) for (int j = 0; j <= i; j++) r[gdg_gram_index((size_t)i, (size_t)j)] = full[(size_t)i * P + j];
    return r;
}

/* the Gram of rows given as vectors of small integers: exact */
static std::vector<double> gram_of(const std::vector<std::vector<double>> &x) {
    const int P = (int)x.size();
    std::vector<double> full((size_t)P * P, 0.0);
    for (int i = 0; i < P; i++) for (int j = 0; j < P; j++) for (size_t k = 0; k < x[i].size(); k++) full[(size_t)i * P + j] += x[i][k] * x[j][k];
    return pack(full, P);
}

int main() {
    /* the section: behind `end`, from the next 16 bytes on, [w] records of P (P + 1) / 2 doubles; no list, no byte */
    int cases = 0, moved = 0;
    for (size_t end : { (size_t)0, (size_t)8, (size_t)16, (size_t)1000, (size_t)4095, (size_t)123457 })
        for (size_t P : { (size_t)0, (size_t)2, (size_t)3, (size_t)64, (size_t)65, (size_t)512 })
            for (size_t w : { (size_t)1, (size_t)2, (size_t)4, (size_t)16 }) {
                const ListShape shape = { 1, gram_record_bytes(P) };
                const ListSection s = list_section(end, shape, w);
                cases++;
                if (P == 0) { CHECK(s.at == end && s.bytes == 0 && s.end == end && list_room(shape, w) == 0); continue; }
                const size_t at = end % 16 ? end + (16 - end % 16) : end, bytes = w * (P * (P + 1) / 2) * 8;
                CHECK(s.at == at && s.bytes == bytes && s.end == at + bytes);
                CHECK(list_room(shape, w) == 16 + bytes && s.end - end <= list_room(shape, w));
                if (at != end) moved++;
            }
    CHECK(gram_record_bytes(512) == 1050624);
    /* the section rides behind the fit section, which rides behind the four kinds' */
    {
        const ReportLive live = { { 32, 0, 40, 0 } };
        const ReportSections sec = report_sections(live, 10, 4, 1001, true);
        const ListSection fit = list_section(sec.end, { 3, FIT_RECORD_BYTES }, 4);
        const ListSection g = list_section(fit.end, { 1, gram_record_bytes(5) }, 4);
        CHECK(g.at == ((fit.end + 15) & ~(size_t)15) && g.at >= fit.at + 3 * 4 * 368 && g.bytes == 4 * 15 * 8);
        const ListSection alone = list_section(list_section(report_sections({ { 0, 0, 0, 0 } }, 10, 4, 1001, true).end, { 0, 0 }, 4).end, { 1, gram_record_bytes(5) }, 4);
        CHECK(alone.at == 1008);
    }

    /* the packed index against a full matrix: every (i, j), j <= i, has its own place, the places are 0 .. P (P + 1) / 2 - 1 by rows */
    for (int P : { 1, 2, 63, 64, 65, 512 }) {
        std::vector<int> seen(gdg_gram_doubles((size_t)P), 0);
        size_t next = 0;
        bool in_order = true;
        for (int i = 0; i < P; i++)
            for (int j = 0; j <= i; j++) {
                const size_t at = gdg_gram_index((size_t)i, (size_t)j);
                if (at != next++) in_order = false;
                if (at < seen.size()) seen[at]++;
            }
        CHECK(in_order && next == seen.size() && next == (size_t)P * ((size_t)P + 1) / 2);
        for (int v : seen) if (v != 1) { CHECK(v == 1); break; }
        std::vector<double> full((size_t)P * P);
        for (int i = 0; i < P; i++) for (int j = 0; j < P; j++) full[(size_t)i * P + j] = (double)((i > j ? i : j) * 1000 + (i > j ? j : i));
        const std::vector<double> r = pack(full, P);
        CHECK(r[gdg_gram_index((size_t)P - 1, 0)] == (double)((P - 1) * 1000) && r.back() == (double)((P - 1) * 1000 + P - 1));
    }

    /* the list's checks */
    {
        const int ok[4] = { 3, 0, 7, 2 }, neg[3] = { 1, -1, 2 }, twice[4] = { 4, 1, 2, 1 };
        int earlier = -1;
        CHECK(gdg_gram_list_bad(ok, 4, 8) == -1 && gdg_gram_list_bad(ok, 4, 7) == 2 && gdg_gram_list_bad(ok, 4, -1) == -1);
        CHECK(gdg_gram_list_bad(neg, 3, -1) == 1);
        CHECK(gdg_gram_list_repeat(ok, 4, &earlier) == -1 && gdg_gram_list_repeat(twice, 4, &earlier) == 3 && earlier == 1);
    }

    int picked[8], n = -5, at = 0;
    double w[8], res[8];
    const double untouched = -7.25;
    auto reset = [&]() { for (int k = 0; k < 8; k++) { picked[k] = -9; w[k] = res[k] = untouched; } n = -5; };
    auto pristine = [&]() { for (int k = 0; k < 8; k++) if (picked[k] != -9 || w[k] != untouched || res[k] != untouched) return false; return n == -5; };

    /* four orthogonal rigs e_0 .. e_3 (list positions 1 .. 4), a silent one (5), a copy of e_1 (6); target (0) = 3 e_1 + 2 e_3 + 1 e_0:
     * T = 14; the first pick is e_1 (leaves 5 / 14), then e_3 (1 / 14), then e_0 (0); the silent rig and the copy are never picked */
    std::vector<std::vector<double>> x = { { 1, 3, 0, 2, 0 }, { 1, 0, 0, 0, 0 }, { 0, 1, 0, 0, 0 }, { 0, 0, 1, 0, 0 }, { 0, 0, 0, 1, 0 }, { 0, 0, 0, 0, 0 }, { 0, 1, 0, 0, 0 } };
    const std::vector<double> G = gram_of(x);
    const int all[6] = { 1, 2, 3, 4, 5, 6 };
    reset();
    CHECK(gdg_blend_pick(G.data(), 7, 1, 0, all, 6, 8, 0.0, 0.0, picked, w, res, &n, &at) == PICK_OK && at == -1);
    CHECK(n == 4 && picked[0] == 2 && picked[1] == 4 && picked[2] == 1);         /* the fourth: e_2, which gains nothing (min_gain 0 lets it in) */
    CHECK(picked[3] == 3 && picked[4] == -1 && w[0] == 3.0 && w[1] == 2.0 && w[2] == 1.0 && w[3] == 0.0 && w[4] == 0.0);
    CHECK(fabs(res[0] - 5.0 / 14.0) <= 1e-15 && fabs(res[1] - 1.0 / 14.0) <= 1e-15 && res[2] == 0.0 && res[3] == 0.0 && res[4] == 0.0);
    /* min_gain stops it where a pick brings too little; max_terms where it says */
    reset();
    CHECK(gdg_blend_pick(G.data(), 7, 1, 0, all, 6, 8, 0.0, 0.1, picked, w, res, &n, &at) == PICK_OK && n == 2 && picked[0] == 2 && picked[1] == 4 && picked[2] == -1);
    CHECK(w[0] == 3.0 && w[1] == 2.0 && w[2] == 0.0);
    reset();
    CHECK(gdg_blend_pick(G.data(), 7, 1, 0, all, 6, 1, 0.0, 0.0, picked, w, res, &n, &at) == PICK_OK && n == 1 && picked[0] == 2 && w[0] == 3.0);
    /* a duplicated candidate: the copy first in the list wins the tie, the other one is then skipped (its pivot is 0), not refused */
    {
        const int copy_first[3] = { 6, 2, 4 };
        reset();
        CHECK(gdg_blend_pick(G.data(), 7, 1, 0, copy_first, 3, 3, 0.0, 0.0, picked, w, res, &n, &at) == PICK_OK && n == 2 && picked[0] == 6 && picked[1] == 4);
    }
    /* only silent candidates: nothing admissible, nothing picked, and that is no error */
    {
        const int silent[1] = { 5 };
        reset();
        CHECK(gdg_blend_pick(G.data(), 7, 1, 0, silent, 1, 3, 0.0, 0.0, picked, w, res, &n, &at) == PICK_OK && n == 0 && picked[0] == -1 && w[0] == 0.0 && res[0] == 0.0);
    }
    /* two blocks are added: the same Gram in halves */
    {
        std::vector<double> two(2 * G.size());
        for (size_t e = 0; e < G.size(); e++) { two[e] = 0.25 * G[e]; two[G.size() + e] = 0.75 * G[e]; }
        reset();
        CHECK(gdg_blend_pick(two.data(), 7, 2, 0, all, 6, 3, 0.0, 0.0, picked, w, res, &n, &at) == PICK_OK && n == 3 && picked[0] == 2 && w[0] == 3.0 && w[2] == 1.0);
    }
    /* the weights are the fit planner's on a fit record with the same sums, bit for bit -- correlated rows, with and without a ridge */
    {
        std::vector<std::vector<double>> y = { { 5, -3, 2, 7, 1, -4 }, { 1, 2, 0, 3, -1, 1 }, { 2, -1, 1, 2, 0, -2 }, { 0, 1, 3, -1, 2, 1 }, { 3, 0, -2, 1, 1, 0 } };
        const std::vector<double> Gy = gram_of(y);
        const int cand[4] = { 1, 2, 3, 4 };
        for (double ridge : { 0.0, 0.01 }) {
            reset();
            CHECK(gdg_blend_pick(Gy.data(), 5, 1, 0, cand, 4, 3, ridge, 0.0, picked, w, res, &n, &at) == PICK_OK && n == 3);
            gdg_blend_fit_rec r;
            memset(&r, 0, sizeof r);
            r.terms = 3;
            r.tt = Gy[gdg_gram_index(0, 0)];
            for (int j = 0; j < 3; j++) {
                r.tx[j] = Gy[gdg_gram_index((size_t)picked[j], 0)];
                for (int k = 0; k <= j; k++) {
                    const size_t a = (size_t)picked[j], b = (size_t)picked[k];
                    r.xx[j * (j + 1) / 2 + k] = a >= b ? Gy[gdg_gram_index(a, b)] : Gy[gdg_gram_index(b, a)];
                }
            }
            double fw[8], fres[1];
            int bad = 0;
            CHECK(gdg_blend_plan_weights(&r, 1, 1, ridge, fw, fres, &bad) == FIT_PLAN_OK);
            CHECK(memcmp(fw, w, sizeof fw) == 0 && memcmp(fres, &res[2], sizeof(double)) == 0);
            CHECK(res[0] >= res[1] && res[1] >= res[2] && res[0] < 1.0);
        }
    }
    /* refusals: nothing is written */
    {
        reset();
        std::vector<double> Z = G;
        Z[gdg_gram_index(0, 0)] = 0.0;
        CHECK(gdg_blend_pick(Z.data(), 7, 1, 0, all, 6, 3, 0.0, 0.0, picked, w, res, &n, &at) == PICK_SILENT && pristine());
        std::vector<double> N = G;
        N[gdg_gram_index(4, 2)] = NAN;
        CHECK(gdg_blend_pick(N.data(), 7, 1, 0, all, 6, 3, 0.0, 0.0, picked, w, res, &n, &at) == PICK_NONFINITE && (at == 2 || at == 4) && pristine());
        const int outside[2] = { 1, 3 };                                         /* ... but a NaN between ports that are no candidates is never read */
        CHECK(gdg_blend_pick(N.data(), 7, 1, 0, outside, 2, 2, 0.0, 0.0, picked, w, res, &n, &at) == PICK_OK && n == 2);
        reset();
        const int twice[3] = { 1, 2, 1 }, is_target[2] = { 1, 0 }, far[2] = { 1, 7 };
        CHECK(gdg_blend_pick(G.data(), 7, 1, 0, twice, 3, 3, 0.0, 0.0, picked, w, res, &n, &at) == PICK_REPEAT && at == 2 && pristine());
        CHECK(gdg_blend_pick(G.data(), 7, 1, 0, is_target, 2, 3, 0.0, 0.0, picked, w, res, &n, &at) == PICK_REPEAT && at == 1 && pristine());
        CHECK(gdg_blend_pick(G.data(), 7, 1, 0, far, 2, 3, 0.0, 0.0, picked, w, res, &n, &at) == PICK_POSITION && at == 1 && pristine());
        CHECK(gdg_blend_pick(G.data(), 7, 1, 7, all, 6, 3, 0.0, 0.0, picked, w, res, &n, &at) == PICK_POSITION && at == -1 && pristine());
        CHECK(gdg_blend_pick(G.data(), 7, 1, 0, all, 6, 9, 0.0, 0.0, picked, w, res, &n, &at) == PICK_ARGS && pristine());
        CHECK(gdg_blend_pick(G.data(), 7, 1, 0, all, 6, 0, 0.0, 0.0, picked, w, res, &n, &at) == PICK_ARGS && pristine());
        CHECK(gdg_blend_pick(G.data(), 7, 0, 0, all, 6, 3, 0.0, 0.0, picked, w, res, &n, &at) == PICK_ARGS && pristine());
        CHECK(gdg_blend_pick(G.data(), 7, 1, 0, all, 6, 3, -1.0, 0.0, picked, w, res, &n, &at) == PICK_ARGS && pristine());
        CHECK(gdg_blend_pick(G.data(), 7, 1, 0, all, 6, 3, 0.0, NAN, picked, w, res, &n, &at) == PICK_ARGS && pristine());
        CHECK(gdg_blend_pick(G.data(), 513, 1, 0, all, 6, 3, 0.0, 0.0, picked, w, res, &n, &at) == PICK_ARGS && pristine());
    }
    if (failures) { printf("%d checks FAILED\n", failures); return 1; }
    printf("OK gram section, index and picks; %d section cases, %d moved by the 16-byte step\n", cases, moved);
    return 0;
}
