/*
 * report_sections_check.cpp -- csrc/report_sections.h driven on the host, without HIP, against a literal restatement of the formulas it
 * replaced: the block loop's cascade of offset lambdas (rec_at / spec_at / align_at / before_tp / tp_at, each at the next 16 bytes behind
 * whatever switch precedes it), the master finish's packed rec_off / spec_off / tp_off, and the slice runner's four *_room terms.  Every
 * offset, size, end and room over the whole grid must be equal.
 * With the real block size (8192) a step's rows end on 16 bytes and so does every section of 32- or 16-byte records: only the section
 * behind an odd count of bands is ever moved.  The grid therefore also walks blocks of 1 and 3 samples, where the rows themselves end
 * anywhere: there the 16-byte step moves every kind's section, and the program counts those cases per kind.
 * Built with -fsanitize=address,undefined by tests/test_report_sections_host.py; prints "OK <cases>" and returns 0, or says what differs.
 */
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "report_sections.h"

static int failures = 0;
static void differ(const char *what, const char *form, size_t got, size_t want, unsigned mask, size_t N, size_t w, size_t width, size_t n_bands, size_t B) {
    if (failures++ < 20)
        printf("FAILED %s (%s): header %zu, restatement %zu; kinds 0x%x, N %zu, w %zu, width %zu, bands %zu, block %zu\n", what, form, got, want, mask, N, w, width, n_bands, B);
}

/* ---- the formulas as they stood, as plain arithmetic -------------------------------------------------------------------------------- */
struct Old { size_t at[4], bytes[4], down; };

/* the block loop (BlockLoop::plan in api_batch.cpp): `down_bytes` = what the step's rows take, `rec_rows` = N + 3 or a shard's N + 1, `w` = the step's blocks */
static Old old_loop(bool report, bool bands, bool align, bool true_peak, size_t down_bytes, size_t rec_rows, size_t w, size_t bands_n) {
    const size_t n_bands = bands ? bands_n : 0;
    const size_t rec_at = (down_bytes + 15) & ~(size_t)15;
    const size_t rec_bytes = rec_rows * w * 32;
    const size_t spec_at = ((report ? rec_at + rec_bytes : down_bytes) + 15) & ~(size_t)15;
    const size_t spec_bytes = rec_rows * w * n_bands * 8;
    const size_t align_at = ((bands ? spec_at + spec_bytes : report ? rec_at + rec_bytes : down_bytes) + 15) & ~(size_t)15;
    const size_t align_bytes = rec_rows * w * 40;                     /* sizeof(gdg_block_align): four doubles, two 32-bit fields */
    const size_t before_tp = align ? align_at + align_bytes : bands ? spec_at + spec_bytes : report ? rec_at + rec_bytes : down_bytes;
    const size_t tp_at = (before_tp + 15) & ~(size_t)15;
    const size_t tp_bytes = rec_rows * w * 16;
    const size_t down = true_peak ? tp_at + tp_bytes : before_tp;
    return Old{ { rec_at, spec_at, align_at, tp_at }, { rec_bytes, spec_bytes, align_bytes, tp_bytes }, down };
}

/* finish_master: a piece of `piece` samples in blocks of B, `width` bytes per encoded sample; no alignment records, no alignment step */
static Old old_finish(bool report, bool bands, bool true_peak, size_t piece, size_t B, size_t width, size_t bands_n) {
    const size_t n_bands = bands ? bands_n : 0;
    const size_t rec_off = 2 * piece * width, rec_bytes = report ? 2 * (piece / B) * 32 : 0;
    const size_t spec_off = rec_off + rec_bytes, spec_bytes = 2 * (piece / B) * n_bands * 8;
    const size_t tp_off = spec_off + spec_bytes, tp_bytes = true_peak ? 2 * (piece / B) * 16 : 0;
    return Old{ { rec_off, spec_off, 0, tp_off }, { rec_bytes, spec_bytes, 0, tp_bytes }, tp_off + tp_bytes };
}

/* run_slice: what the four kinds add to a half for a window of W blocks */
static size_t old_room(bool report, bool bands, bool align, bool true_peak, size_t rows, size_t W, size_t n_bands) {
    const size_t rec_room = report ? 16 + rows * W * 32 : 0;
    const size_t spec_room = bands ? 16 + rows * W * n_bands * 8 : 0;
    const size_t align_room = align ? 16 + rows * W * 40 : 0;
    const size_t tp_room = true_peak ? 16 + rows * W * 16 : 0;
    return rec_room + spec_room + align_room + tp_room;
}

int main() {
    size_t cases = 0, moved[REPORT_KINDS] = { 0, 0, 0, 0 };
    for (unsigned mask = 0; mask < 16; mask++) {
        const bool on[4] = { (mask & 1) != 0, (mask & 2) != 0, (mask & 4) != 0, (mask & 8) != 0 };
        for (size_t n_bands : { 1, 2, 31 })
        for (size_t N : { 1, 3, 8, 512 })
        for (size_t w : { 1, 2, 4, 16 })
        for (size_t width : { 2, 3, 4, 8 })
        for (size_t B : { 8192, 1, 3 }) {
            ReportLive live;
            for (int k = 0; k < REPORT_KINDS; k++) live.elem[k] = on[k] ? report_elem(k, n_bands) : 0;
            const size_t wb = w * B, row_bytes = wb * width;
            auto hold = [&](const char *form, const ReportSections &s, const Old &o, size_t base, bool aligned) {
                size_t prev = base;                                          /* where the section would start without the 16-byte step */
                for (int k = 0; k < REPORT_KINDS; k++) {
                    if (!live.on(k)) continue;
                    if (s.at[k] != o.at[k]) differ("offset", form, s.at[k], o.at[k], mask, N, w, width, n_bands, B);
                    if (s.bytes[k] != o.bytes[k]) differ("size", form, s.bytes[k], o.bytes[k], mask, N, w, width, n_bands, B);
                    if (aligned && o.at[k] != prev) moved[k]++;
                    prev = o.at[k] + o.bytes[k];
                }
                if (s.end != o.down) differ("end", form, s.end, o.down, mask, N, w, width, n_bands, B);
                cases++;
            };
            auto hold_room = [&](const char *form, size_t rows) {
                for (size_t W : { w, (size_t)16, (size_t)64 }) {
                    if (W < w) continue;
                    const size_t got = report_room(live, rows, W), want = old_room(on[0], on[1], on[2], on[3], rows, W, n_bands);
                    if (got != want) differ("room", form, got, want, mask, N, W, width, n_bands, B);
                }
            };
            /* a plain call: N + 3 rows, every one encoded */
            {
                const size_t NO = N + 3, down_bytes = NO * row_bytes;
                hold("plain", report_sections(live, NO, w, down_bytes, true), old_loop(on[0], on[1], on[2], on[3], down_bytes, NO, w, n_bands), down_bytes, true);
                hold_room("plain", NO);
            }
            /* a shard: N + 1 record rows; its encoded rows with and without the metronome's, its float64 rows likewise */
            for (size_t enc_rows : { N, N + 1 })
            for (size_t f64_rows : { 2, 3 }) {
                const size_t down_bytes = ((enc_rows * row_bytes + 15) & ~(size_t)15) + f64_rows * wb * sizeof(double);
                hold("shard", report_sections(live, N + 1, w, down_bytes, true), old_loop(on[0], on[1], on[2], on[3], down_bytes, N + 1, w, n_bands), down_bytes, true);
                hold_room("shard", N + 1);
            }
            /* a finish over G = N shards: two rows, pieces of w blocks and of the size the finish picks; never alignment records */
            if (!on[REPORT_ALIGN]) {
                const size_t G = N, picked = B * std::min((size_t)128, std::max((size_t)1, ((size_t)8 << 20) / ((2 * G + 1) * B * sizeof(double))));
                for (size_t piece : { wb, picked })
                    hold("finish", report_sections(live, 2, piece / B, 2 * piece * width, false), old_finish(on[0], on[1], on[3], piece, B, width, n_bands), 2 * piece * width, false);
            }
        }
    }
    /* non-vacuity: the grid is at least 16 kinds x 3 forms x 4 N x 4 w x 4 widths x 3 band counts, and the 16-byte step has moved every kind's section */
    const size_t least = (size_t)16 * 3 * 4 * 4 * 4 * 3;
    if (cases < least) { printf("FAILED: %zu cases, the grid has at least %zu\n", cases, least); failures++; }
    for (int k = 0; k < REPORT_KINDS; k++)
        if (moved[k] == 0) { printf("FAILED: the 16-byte step never moved kind %d's section\n", k); failures++; }
    if (failures) return 1;
    printf("OK %zu cases; sections moved by the 16-byte step: %zu %zu %zu %zu\n", cases, moved[0], moved[1], moved[2], moved[3]);
    return 0;
}
