/*
 * transfer_plan_check.cpp -- the transfer records without HIP (csrc/report_sections.h, csrc/blend.h).  THE SECTION: with each of the 16
 * on/off combinations of the three list kinds in front and the transfer list, for w = 1, 3 and 16 blocks, the transfer section starts at the
 * next 16 bytes behind the three kinds' end, holds w records, and the three kinds' sections are where they are without a transfer list.  THE LIST: what
 * gdg_transfer_check refuses, the table a launch reads and the record's size.  THE PLANNER: the filter {1, -2, 3} from records synthesised
 * with Sxx = 1, Syy = |H|^2, Sxy = H -- the taps under the taper at center 0 and shifted at center 5, coherence 1 -- its refusals, which
 * write nothing, and the ridge, which shrinks every |H[g]| and with it the taps' energy.  Built by tests/test_transfer_host.py.
 */
#include "report_sections.h"
#include "blend.h"

#include <cmath>
#include <cstdio>
#include <vector>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static std::vector<double> synth(const std::vector<double> &h, int D) {
    const int G = 4096 / D + 1, M = 2 * (G - 1);
    const double pi = 3.14159265358979323846;
    std::vector<double> rec((size_t)G * 4);
    for (int g = 0; g < G; g++) {
        double re = 0.0, im = 0.0;
        for (size_t m = 0; m < h.size(); m++) { re += h[m] * cos(2.0 * pi * g * (double)m / M); im -= h[m] * sin(2.0 * pi * g * (double)m / M); }
        if (g == 0 || g == G - 1) im = 0.0;
        rec[(size_t)g * 4] = 1.0; rec[(size_t)g * 4 + 1] = re * re + im * im; rec[(size_t)g * 4 + 2] = re; rec[(size_t)g * 4 + 3] = im;
    }
    return rec;
}

int main() {
    /* ---- the section ---- */
    int cases = 0, moved = 0;
    for (int mask = 0; mask < 16; mask++)
        for (size_t w : { (size_t)1, (size_t)3, (size_t)16 })
            for (size_t base : { (size_t)0, (size_t)4 * 8192 * 2 * w + 8, (size_t)1000003 }) {
                const ListShape transfer = { 1, (mask & 8) ? transfer_record_bytes(2, 32) : 0 };
                const ListShape shape[LIST_KINDS] = { { (size_t)((mask & 1) ? 2 : 0), (size_t)((mask & 1) ? FIT_RECORD_BYTES : 0) }, { 1, (mask & 2) ? gram_record_bytes(3) : 0 },
                                                      { 1, (mask & 4) ? (size_t)21 * 8 : 0 }, transfer, { 0, 0 } };      /* the delivered rows' records: off */
                const ListSections all = list_sections(base, shape, w);
                const ListSection t = all.of[LIST_TRANSFER];
                CHECK(all.of[LIST_DELIVERED].bytes == 0 && all.of[LIST_DELIVERED].at == t.end && all.end == t.end);
                struct { const ListSection *of; size_t end; } lists = { all.of, all.of[LIST_TAPFIT].end };      /* the three kinds in front, and their end */
                size_t end = base;                                             /* the three kinds, by hand: a fourth behind them moves none of them */
                for (int k = 0; k < LIST_TRANSFER; k++) {
                    if (!shape[k].on()) { CHECK(lists.of[k].bytes == 0 && lists.of[k].end == end); continue; }
                    const size_t at = (end + 15) / 16 * 16;
                    CHECK(lists.of[k].at == at && lists.of[k].bytes == shape[k].rows * w * shape[k].elem);
                    end = at + lists.of[k].bytes;
                }
                CHECK(lists.end == end);
                if (mask & 8) {
                    CHECK(t.at == (lists.end + 15) / 16 * 16 && t.at % 16 == 0 && t.at - lists.end < 16);
                    CHECK(t.bytes == w * 2 * (4096 / 32 + 1) * 4 * 8 && t.end == t.at + t.bytes);
                    CHECK(list_room(transfer, w) == 16 + t.bytes && t.end - lists.end <= list_room(transfer, w));
                    if (t.at != lists.end) moved++;
                } else {
                    CHECK(t.at == lists.end && t.bytes == 0 && t.end == lists.end && list_room(transfer, w) == 0);
                }
                cases++;
            }
    CHECK(transfer_record_bytes(1, 1) == 131104 && transfer_record_bytes(0, 1) == 0 && transfer_record_bytes(16, 64) == 16 * 65 * 32);
    static_assert(LIST_TRANSFER == 3 && LIST_DELIVERED == 4 && LIST_KINDS == 5, "the transfer list is the fourth entry of the chain, behind the three kinds");

    /* ---- the list ---- */
    int pair = -2;
    const int port[3] = { 0, 5, 2 }, target[3] = { 1, 1, 9 };
    CHECK(gdg_transfer_check(3, port, target, 32, 10, &pair) == TRANSFER_OK && pair == -1);
    CHECK(gdg_transfer_check(3, port, target, 32, -1, &pair) == TRANSFER_OK);
    CHECK(gdg_transfer_check(3, port, target, 32, 9, &pair) == TRANSFER_TARGET && pair == 2);
    CHECK(gdg_transfer_check(3, port, target, 32, 5, &pair) == TRANSFER_PORT && pair == 1);
    CHECK(gdg_transfer_check(17, port, target, 32, 10, &pair) == TRANSFER_COUNT && gdg_transfer_check(-1, port, target, 32, 10, &pair) == TRANSFER_COUNT);
    CHECK(gdg_transfer_check(3, nullptr, target, 32, 10, &pair) == TRANSFER_NULL && gdg_transfer_check(0, nullptr, nullptr, 0, 10, &pair) == TRANSFER_OK);
    for (int D : { 0, 3, 128, -4, 48 }) CHECK(gdg_transfer_check(3, port, target, D, 10, &pair) == TRANSFER_GROUP);
    for (int D : { 1, 2, 4, 8, 16, 32, 64 }) CHECK(gdg_transfer_check(3, port, target, D, 10, &pair) == TRANSFER_OK && gdg_transfer_list_doubles(3, D) == (size_t)3 * (4096 / D + 1) * 4);
    const std::vector<int> table = gdg_transfer_table(3, port, target, 8);
    CHECK(table == (std::vector<int>{ 0, 1, 5, 1, 2, 9, 8 }) && gdg_transfer_table(0, nullptr, nullptr, 8).empty());
    TransferSet set;
    CHECK(set.count() == 0 && set.doubles() == 0 && set.group() == 0);
    set.table = table;
    int side = -1;
    CHECK(set.count() == 3 && set.group() == 8 && set.doubles() == (size_t)3 * 513 * 4 && set.first_outside(10, &side) == -1 && set.first_outside(9, &side) == 2 && side == 1);
    CHECK(set.first_outside(5, &side) == 1 && side == 0);

    /* ---- the planner ---- */
    const double pi = 3.14159265358979323846;
    for (int D : { 1, 8, 64 }) {
        const std::vector<double> rec = synth({ 1.0, -2.0, 3.0 }, D);
        const int n_taps = 16;
        for (int center : { 0, 5 }) {
            std::vector<double> tap((size_t)n_taps, 99.0);
            double coh = 99.0;
            CHECK(gdg_match_plan_taps(rec.data(), 1, D, 1, 0.0, n_taps, center, tap.data(), &coh, &pair) == MATCH_PLAN_OK && pair == -1);
            const double h[3] = { 1.0, -2.0, 3.0 };
            for (int m = 0; m < n_taps; m++) {
                const int d = m - center;
                const double E = d < 0 ? center + 1.0 : (double)(n_taps - center), t = 0.5 + 0.5 * cos(pi * d / E);
                const double want = (d >= 0 && d < 3) ? t * h[d] : 0.0;
                CHECK(fabs(tap[(size_t)m] - want) <= 1e-13);
                CHECK(t > 0.0);
            }
            CHECK(tap[(size_t)center] == tap[(size_t)center] && fabs(tap[(size_t)center] - 1.0) <= 1e-13 && fabs(coh - 1.0) <= 1e-13);
        }
        /* the ridge: every |H[g]| shrinks (Sxx = 1 everywhere: by 1 / (1 + ridge)), and the taps' energy with it */
        std::vector<double> a(16), b(16);
        double ca = 0.0, cb = 0.0, ea = 0.0, eb = 0.0;
        CHECK(gdg_match_plan_taps(rec.data(), 1, D, 1, 0.0, 16, 0, a.data(), &ca, &pair) == MATCH_PLAN_OK && gdg_match_plan_taps(rec.data(), 1, D, 1, 0.25, 16, 0, b.data(), &cb, &pair) == MATCH_PLAN_OK);
        for (int m = 0; m < 16; m++) { ea += a[(size_t)m] * a[(size_t)m]; eb += b[(size_t)m] * b[(size_t)m]; }
        CHECK(eb < ea && fabs(eb - ea / (1.25 * 1.25)) <= 1e-12 * ea && ca == cb);
        /* refusals: nothing is written */
        std::vector<double> tap(16, 99.0);
        double coh = 99.0;
        auto untouched = [&] { for (double v : tap) if (v != 99.0) return false; return coh == 99.0; };
        std::vector<double> bad = rec;
        bad[7] = NAN;
        CHECK(gdg_match_plan_taps(bad.data(), 1, D, 1, 0.0, 16, 0, tap.data(), &coh, &pair) == MATCH_PLAN_NONFINITE && pair == 0 && untouched());
        bad = rec;
        for (size_t g = 0; g < bad.size() / 4; g++) bad[g * 4] = 0.0;
        CHECK(gdg_match_plan_taps(bad.data(), 1, D, 1, 0.0, 16, 0, tap.data(), &coh, &pair) == MATCH_PLAN_SILENT && pair == 0 && untouched());
        const int half = 4096 / D;
        CHECK(gdg_match_plan_taps(rec.data(), 1, D, 1, 0.0, half + 1, 0, tap.data(), &coh, &pair) == MATCH_PLAN_ARGS && untouched());
        CHECK(gdg_match_plan_taps(rec.data(), 1, D, 1, 0.0, 16, 16, tap.data(), &coh, &pair) == MATCH_PLAN_ARGS && untouched());
        CHECK(gdg_match_plan_taps(rec.data(), 1, D, 1, 0.0, 16, -1, tap.data(), &coh, &pair) == MATCH_PLAN_ARGS && untouched());
        CHECK(gdg_match_plan_taps(rec.data(), 1, 3, 1, 0.0, 16, 0, tap.data(), &coh, &pair) == MATCH_PLAN_ARGS && untouched());
        CHECK(gdg_match_plan_taps(rec.data(), 1, D, 0, 0.0, 16, 0, tap.data(), &coh, &pair) == MATCH_PLAN_ARGS && untouched());
        CHECK(gdg_match_plan_taps(rec.data(), 1, D, 1, -1.0, 16, 0, tap.data(), &coh, &pair) == MATCH_PLAN_ARGS && untouched());
    }
    /* two pairs, the second silent: the first one's taps are not written either */
    {
        std::vector<double> rec = synth({ 1.0, -2.0, 3.0 }, 64), two(rec);
        two.insert(two.end(), rec.size(), 0.0);
        std::vector<double> tap(32, 99.0), coh(2, 99.0);
        CHECK(gdg_match_plan_taps(two.data(), 2, 64, 1, 0.0, 16, 0, tap.data(), coh.data(), &pair) == MATCH_PLAN_SILENT && pair == 1 && tap[0] == 99.0 && coh[0] == 99.0);
    }
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("OK transfer section, list and planner; %d section cases, %d moved by the 16-byte step\n", cases, moved);
    return 0;
}
