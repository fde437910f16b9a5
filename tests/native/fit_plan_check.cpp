/*
 * fit_plan_check.cpp -- the blend fit's host arithmetic without HIP: the planner of csrc/blend.h (gdg_blend_plan_weights) against hand-made
 * records whose answers are known in closed form, the list's validation (gdg_fit_check, gdg_fit_table), and the place and room of the fit
 * section in a step's download half (csrc/report_sections.h: list_section, list_room with the fits' shape) against the formula spelled out
 * here, over the on/off combinations of the four record kinds; and the chain of the three list sections behind a report layout, over the
 * 8 on/off subsets of the lists.  Built by tests/test_fit_host.py, once more under AddressSanitizer and UBSan.
 */
#include "blend.h"
#include "report_sections.h"

#include <cstdio>
#include <cstdlib>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static bool near(double a, double b, double tol) { return fabs(a - b) <= tol; }

/* a record of K terms from a Gram matrix, b and T */
static gdg_blend_fit_rec record(int K, double T, const double *b, const double *G /* [K][K] */) {
    gdg_blend_fit_rec r;
    memset(&r, 0, sizeof r);
    r.tt = T;
    for (int j = 0; j < K; j++) {
        r.tx[j] = b[j];
        for (int k = 0; k <= j; k++) r.xx[j * (j + 1) / 2 + k] = G[j * K + k];
    }
    r.terms = (uint32_t)K;
    return r;
}

int main() {
    static_assert(sizeof(gdg_blend_fit_rec) == 368 && FIT_RECORD_BYTES == 368, "a fit record is 368 bytes");
    double w[2 * 8], res[2];
    int bad = 0;
    const double untouched = -7.25;
    auto reset = [&]() { for (double &v : w) v = untouched; res[0] = res[1] = untouched; };

    /* K = 1: w = b / G, and the tail weights are 0 */
    {
        const double b[1] = { 2.0 }, G[1] = { 4.0 };
        const gdg_blend_fit_rec r = record(1, 3.0, b, G);
        reset();
        CHECK(gdg_blend_plan_weights(&r, 1, 1, 0.0, w, res, &bad) == FIT_PLAN_OK && bad == -1);
        CHECK(w[0] == 0.5);
        for (int k = 1; k < 8; k++) CHECK(w[k] == 0.0);
        CHECK(near(res[0], (3.0 - 2.0 * 0.5 * 2.0 + 0.25 * 4.0) / 3.0, 1e-15));      /* (T - 2 w b + w G w) / T = 2/3 */
        CHECK(w[8] == untouched && res[1] == untouched);                             /* one fit: one row written */
    }
    /* K = 2, orthogonal terms, the records of two blocks added: G = diag(4, 1), b = {2, 3}, T = 10: w = {0.5, 3}, nothing left */
    {
        const double b0[2] = { 1.5, 1.0 }, b1[2] = { 0.5, 2.0 }, G0[4] = { 1.0, 0.0, 0.0, 0.75 }, G1[4] = { 3.0, 0.0, 0.0, 0.25 };
        const gdg_blend_fit_rec r[2] = { record(2, 4.0, b0, G0), record(2, 6.0, b1, G1) };
        reset();
        CHECK(gdg_blend_plan_weights(r, 1, 2, 0.0, w, res, &bad) == FIT_PLAN_OK);
        CHECK(w[0] == 0.5 && w[1] == 3.0 && w[2] == 0.0 && w[7] == 0.0 && res[0] == 0.0);
    }
    /* the target is term 0 of three correlated terms: w = e_0, residual 0 within 1e-10 */
    {
        const double G[9] = { 2.0, 0.5, -0.25, 0.5, 1.0, 0.125, -0.25, 0.125, 3.0 }, b[3] = { 2.0, 0.5, -0.25 };
        const gdg_blend_fit_rec r = record(3, 2.0, b, G);
        reset();
        CHECK(gdg_blend_plan_weights(&r, 1, 1, 0.0, w, res, &bad) == FIT_PLAN_OK);
        CHECK(near(w[0], 1.0, 1e-14) && near(w[1], 0.0, 1e-14) && near(w[2], 0.0, 1e-14) && w[3] == 0.0);
        CHECK(res[0] >= 0.0 && res[0] <= 1e-10);
    }
    /* one port twice: refused without a ridge, outputs untouched and the fit named; equal weights with one */
    {
        const double G[4] = { 4.0, 4.0, 4.0, 4.0 }, b[2] = { 2.0, 2.0 }, G1[1] = { 1.0 }, b1[1] = { 1.0 };
        const gdg_blend_fit_rec r[2] = { record(1, 1.0, b1, G1), record(2, 1.0, b, G) };      /* fit 0 is fine, fit 1 is the offender */
        reset();
        CHECK(gdg_blend_plan_weights(r, 2, 1, 0.0, w, res, &bad) == FIT_PLAN_PIVOT && bad == 1);
        for (double v : w) CHECK(v == untouched);
        CHECK(res[0] == untouched && res[1] == untouched);
        CHECK(gdg_blend_plan_weights(r, 2, 1, 1e-3, w, res, &bad) == FIT_PLAN_OK && bad == -1);
        CHECK(near(w[8], w[9], 1e-12) && near(w[8], 2.0 / (8.0 + 4.0e-3), 1e-12));   /* (4 + 4 + 4 ridge) w = 2 */
        CHECK(near(w[0], 1.0 / 1.001, 1e-14));
    }
    /* a silent term is a zero pivot; a silent target gives zero weights and residual 0 */
    {
        const double G[4] = { 4.0, 0.0, 0.0, 0.0 }, b[2] = { 2.0, 0.0 };
        const gdg_blend_fit_rec r = record(2, 1.0, b, G);
        reset();
        CHECK(gdg_blend_plan_weights(&r, 1, 1, 0.0, w, res, &bad) == FIT_PLAN_PIVOT && bad == 0 && w[0] == untouched);
        const double G2[4] = { 4.0, 1.0, 1.0, 2.0 }, b2[2] = { 0.0, 0.0 };
        const gdg_blend_fit_rec z = record(2, 0.0, b2, G2);
        CHECK(gdg_blend_plan_weights(&z, 1, 1, 0.0, w, res, &bad) == FIT_PLAN_OK && w[0] == 0.0 && w[1] == 0.0 && res[0] == 0.0);
    }
    /* what the arguments refuse: a negative or non-finite ridge, no block, records that disagree on K or hold none */
    {
        const double G[1] = { 1.0 }, b[1] = { 1.0 };
        gdg_blend_fit_rec r[2] = { record(1, 1.0, b, G), record(1, 1.0, b, G) };
        CHECK(gdg_blend_plan_weights(r, 1, 2, -1.0, w, res, &bad) == FIT_PLAN_ARGS);
        CHECK(gdg_blend_plan_weights(r, 1, 2, NAN, w, res, &bad) == FIT_PLAN_ARGS);
        CHECK(gdg_blend_plan_weights(r, 1, 2, INFINITY, w, res, &bad) == FIT_PLAN_ARGS);
        CHECK(gdg_blend_plan_weights(r, 1, 0, 0.0, w, res, &bad) == FIT_PLAN_ARGS);
        CHECK(gdg_blend_plan_weights(r, 0, 0, 0.0, nullptr, nullptr, &bad) == FIT_PLAN_OK);
        r[1].terms = 2;
        CHECK(gdg_blend_plan_weights(r, 1, 2, 0.0, w, res, &bad) == FIT_PLAN_TERMS && bad == 0);
        r[0].terms = 9;
        CHECK(gdg_blend_plan_weights(r, 1, 1, 0.0, w, res, &bad) == FIT_PLAN_TERMS);
    }
    /* the list: CSR form into the table the kernel reads */
    {
        const int first[3] = { 0, 2, 5 }, port[5] = { 0, 1, 4, 4, 2 }, target[2] = { 6, 0 };
        int f = 0, k = 0;
        CHECK(gdg_fit_check(2, first, port, target, 7, &f, &k) == FIT_OK && f == -1);
        CHECK(gdg_fit_check(2, first, port, target, 6, &f, &k) == FIT_TARGET && f == 0);
        CHECK(gdg_fit_check(2, first, port, target, -1, &f, &k) == FIT_OK);
        const int low[5] = { 0, 1, 4, -1, 2 };
        CHECK(gdg_fit_check(2, first, low, target, -1, &f, &k) == FIT_PORT && f == 1 && k == 1);
        const int none[3] = { 0, 0, 5 }, nine[2] = { 0, 9 };
        CHECK(gdg_fit_check(2, none, port, target, 7, &f, &k) == FIT_TERMS && f == 0);
        CHECK(gdg_fit_check(1, nine, port, target, 7, &f, &k) == FIT_TERMS && f == 0);
        CHECK(gdg_fit_check(GDG_FIT_MAX_FITS + 1, first, port, target, 7, &f, &k) == FIT_COUNT);
        FitSet set;
        set.table = gdg_fit_table(2, first, port, target);
        CHECK(set.count() == 2 && set.target(0) == 6 && set.terms(0) == 2 && set.terms(1) == 3 && set.port(1, 2) == 2 && set.port(0, 1) == 1);
        CHECK(set.table.size() == 20 && set.table[4] == 0 && set.table[19] == 0);
        CHECK(set.first_outside(7, &k) == -1);
        CHECK(set.first_outside(6, &k) == 0 && k == -1);
        CHECK(set.first_outside(4, &k) == 0 && k == -1);
        set.table[0] = 0;
        CHECK(set.first_outside(4, &k) == 1 && k == 0);
    }
    /* the fit section: behind the end of the last live kind's section -- behind the rows when none is live -- moved up to the next 16
     * bytes, [fits][w] records of 368 bytes; the room is that for a window and the 16 bytes of the move.  Spelled out, not restated. */
    size_t cases = 0, moved = 0;
    for (int mask = 0; mask < 16; mask++)
        for (size_t rows : { (size_t)4, (size_t)9, (size_t)515 })
            for (size_t w : { (size_t)1, (size_t)2, (size_t)4, (size_t)16 })
                for (size_t width : { (size_t)1, (size_t)2, (size_t)3, (size_t)8 })
                    for (size_t n_bands : { (size_t)1, (size_t)7 })
                        for (size_t fits : { (size_t)0, (size_t)1, (size_t)3, (size_t)256 }) {
                            ReportLive live;
                            for (int k = 0; k < REPORT_KINDS; k++) live.elem[k] = (mask >> k) & 1 ? report_elem(k, n_bands) : 0;
                            const size_t base = rows * w * 8192 * width + (width == 3 ? 8 : 0);      /* an end that is no multiple of 16 */
                            const ReportSections sec = report_sections(live, rows, w, base, true);
                            size_t end = base;                                       /* the cascade, by hand */
                            if (mask & 1) end = ((end + 15) / 16) * 16 + rows * w * 32;
                            if (mask & 2) end = ((end + 15) / 16) * 16 + rows * w * n_bands * 8;
                            if (mask & 4) end = ((end + 15) / 16) * 16 + rows * w * 40;
                            if (mask & 8) end = ((end + 15) / 16) * 16 + rows * w * 16;
                            CHECK(sec.end == end);
                            const ListShape shape = { fits, fits ? (size_t)FIT_RECORD_BYTES : 0 };
                            const ListSection fs = list_section(sec.end, shape, w);
                            if (fits == 0) CHECK(fs.at == end && fs.bytes == 0 && fs.end == end && list_room(shape, w) == 0);
                            else {
                                const size_t at = ((end + 15) / 16) * 16;
                                CHECK(fs.at == at && fs.bytes == fits * w * 368 && fs.end == at + fits * w * 368);
                                CHECK(list_room(shape, w) == 16 + fits * w * 368);
                                CHECK(fs.end - base <= report_room(live, rows, w) + list_room(shape, w));      /* a step of the whole window fits its half */
                                if (at != end) moved++;
                            }
                            cases++;
                        }
    CHECK(moved > 0);
    /* the chain of the list sections (list_sections) behind a report layout, over the 8 on/off subsets of the first three lists: every live
     * section starts at the next 16 bytes behind what precedes it, an off kind takes no byte and moves nothing, and a step of the whole
     * window fits the room of its half.  3 fits, a Gram list of 5 ports, tap fits of 21 doubles. */
    {
        static_assert(LIST_FIT == 0 && LIST_GRAM == 1 && LIST_TAPFIT == 2 && LIST_TRANSFER == 3 && LIST_DELIVERED == 4 && LIST_KINDS == 5, "the sections ride in this order");
        const size_t elem[LIST_KINDS] = { 368, 5 * 6 / 2 * 8, 21 * 8, 0, 0 }, rows[LIST_KINDS] = { 3, 1, 1, 1, 7 };      /* the last two kinds stay off here (`on` < 8) */
        CHECK(gram_record_bytes(5) == elem[LIST_GRAM]);
        for (int report = 0; report < 2; report++)
            for (size_t base : { (size_t)0, (size_t)1001, (size_t)4096, (size_t)98312 })
                for (size_t w : { (size_t)1, (size_t)2, (size_t)16 })
                    for (int on = 0; on < 8; on++) {
                        const ReportLive live = { { report ? (size_t)32 : 0, 0, report ? (size_t)40 : 0, 0 } };
                        const ReportSections sec = report_sections(live, 7, w, base, true);
                        ListShape shape[LIST_KINDS];
                        for (int k = 0; k < LIST_KINDS; k++) shape[k] = { rows[k], (on >> k) & 1 ? elem[k] : 0 };
                        const ListSections ls = list_sections(sec.end, shape, w);
                        size_t end = sec.end, room = report_room(live, 7, w);
                        for (int k = 0; k < LIST_KINDS; k++) {
                            const ListSection &s = ls.of[k];
                            if ((on >> k) & 1) {
                                CHECK(s.at == (end + 15) / 16 * 16 && s.bytes == rows[k] * w * elem[k] && s.end == s.at + s.bytes);
                                end = s.end;
                            } else CHECK(s.at == end && s.bytes == 0 && s.end == end && list_room(shape[k], w) == 0);
                            room += list_room(shape[k], w);
                        }
                        CHECK(ls.end == end && ls.end - base <= room);
                        if (!on) CHECK(ls.end == sec.end);
                    }
    }
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("OK planner and list; %zu section cases, %zu moved by the 16-byte step\n", cases, moved);
    return 0;
}
