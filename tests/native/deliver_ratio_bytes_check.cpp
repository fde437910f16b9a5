/*
 * deliver_ratio_bytes_check.cpp -- the byte counts of a batch step delivered at factor R and ratio L / M (csrc/deliver.h) against plain
 * formulas: the delivered count, the pitch, the bytes the scatter copies, where a step's bytes lie in a port's file, rows_end and the window's
 * room -- for jobs cut into steps and slices -- and ratio 1/1 against the figures tests/native/deliver_bytes_check.cpp holds.  A program of
 * its own: it needs no device and no HIP header, and may be built with -fsanitize=address,undefined.
 *   g++ -std=c++17 -Wall -I go-dsp-guitar_amd/csrc tests/native/deliver_ratio_bytes_check.cpp -o deliver_ratio_bytes_check && ./deliver_ratio_bytes_check
 */
#include "deliver.h"
#include "report_sections.h"

#include <stdio.h>
#include <initializer_list>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

typedef unsigned long long u64;
static u64 ceil_div(u64 a, u64 b) { return a / b + (a % b ? 1 : 0); }

int main() {
    /* the rules */
    CHECK(gdg_deliver_ratio_ok(147, 160) && gdg_deliver_ratio_ok(160, 147) && gdg_deliver_ratio_ok(1, 1) && gdg_deliver_ratio_ok(1, 2) && gdg_deliver_ratio_ok(2, 1) && gdg_deliver_ratio_ok(160, 319));
    CHECK(!gdg_deliver_ratio_ok(294, 320) && !gdg_deliver_ratio_ok(2, 2) && !gdg_deliver_ratio_ok(1, 3) && !gdg_deliver_ratio_ok(3, 1) && !gdg_deliver_ratio_ok(161, 160) &&
          !gdg_deliver_ratio_ok(147, 320) && !gdg_deliver_ratio_ok(0, 1) && !gdg_deliver_ratio_ok(1, 0) && !gdg_deliver_ratio_ok(-1, 1) && !gdg_deliver_ratio_ok(160, 321));
    CHECK(gdg_deliver_ratio_tap_count(147, 160) == 70 && gdg_deliver_ratio_tap_count(160, 147) == 64 && gdg_deliver_ratio_tap_count(1, 2) == 128 && gdg_deliver_ratio_tap_count(2, 3) == 96 &&
          gdg_deliver_ratio_tap_count(1, 1) == 0 && gdg_deliver_ratio_tap_count(2, 2) == 0);
    for (int L = 1; L <= 160; L++)
        for (int M = 1; M <= 320; M++)
            if (gdg_deliver_ratio_ok(L, M) && gdg_deliver_ratio_on(L, M)) {
                const int T = gdg_deliver_ratio_tap_count(L, M);
                CHECK(T % 2 == 0 && T >= 64 && T <= GDG_DELIVER_RATIO_MAX_TAPS && T - 1 <= GDG_DELIVER_RATIO_HISTORY);
                CHECK(T / 2 == (M <= L ? 32 : (int)ceil_div(32ull * (u64)M, (u64)L)));
                CHECK(255ull * (u64)M / (u64)L + 1 + (u64)T <= 640);                /* a tile's window, the even slot in front included */
            }
    CHECK(gdg_deliver_ratio_latency(4, 147, 160) == 77 + 4 * 35 && gdg_deliver_ratio_latency(2, 160, 147) == 38 + 2 * 32 && gdg_deliver_ratio_latency(1, 147, 160) == 35 &&
          gdg_deliver_ratio_latency(4, 1, 1) == 77 && gdg_deliver_ratio_latency(1, 1, 1) == 0 && gdg_deliver_ratio_latency(3, 147, 160) == 0 && gdg_deliver_ratio_latency(2, 2, 2) == 0);
    CHECK(gdg_deliver_samples(1, 147, 160, 0, 8192) == 7527 && gdg_deliver_samples(1, 147, 160, 8192, 8192) == 7526 && gdg_deliver_samples(4, 147, 160, 0, 4 * 160) == 147);
    CHECK(gdg_deliver_samples(1, 160, 147, 0, 147) == 160 && gdg_deliver_samples(1, 1, 2, 0, 1) == 1 && gdg_deliver_samples(1, 1, 2, 1, 1) == 0);

    const size_t widths[] = { 1, 2, 3, 4, 8 };
    const size_t rows = 7;
    const ReportLive live = { { 32, 3 * 8, 0, 16 } };
    const int ratios[][2] = { { 1, 1 }, { 147, 160 }, { 160, 147 }, { 2, 3 }, { 3, 2 }, { 1, 2 }, { 2, 1 } };
    int cases = 0;
    for (int R : { 1, 2, 4 })
        for (const auto &q : ratios)
            for (size_t W : { (size_t)1, (size_t)4 })
                for (size_t width : widths) {
                    const int L = q[0], M = q[1];
                    /* a job of 7 blocks in slices of 3, 3 and 1 blocks, each in steps of W blocks: the files fill without a gap or an overlap */
                    const size_t job = 7;
                    u64 delivered = 0;
                    for (size_t pos = 0; pos < job; pos += 3) {
                        const size_t slice = pos + 3 <= job ? 3 : job - pos;
                        size_t file_end = 0;
                        for (size_t first = 0; first < slice; first += W) {
                            const size_t w = first + W <= slice ? W : slice - first, off = first * 8192;
                            const DeliverStep s = deliver_ratio_step(w, off, pos * 8192, R, L, M, width, rows);
                            const u64 s0 = (u64)(pos * 8192 + off) / (u64)R, s1 = s0 + (u64)w * 8192 / (u64)R;
                            CHECK(s.inter_first == s0 && s.inter_samples == s1 - s0);
                            CHECK(s.first_out == ceil_div(s0 * (u64)L, (u64)M));
                            CHECK(s.samples == ceil_div(s1 * (u64)L, (u64)M) - ceil_div(s0 * (u64)L, (u64)M));
                            CHECK(s.pitch % 4 == 0 && s.pitch >= s.samples && s.pitch < s.samples + 4);
                            CHECK(s.row_bytes == s.pitch * width && s.row_bytes % 4 == 0 && s.copy_bytes == s.samples * width && s.copy_bytes <= s.row_bytes);
                            CHECK(s.file_at == file_end);
                            CHECK(s.file_at == (s.first_out - ceil_div((u64)(pos * 8192) / (u64)R * (u64)L, (u64)M)) * width);
                            CHECK(s.rows_end == rows * s.row_bytes);
                            file_end = s.file_at + s.copy_bytes;
                            const ReportSections sec = report_sections(live, rows, w, s.rows_end, true);
                            CHECK(sec.at[REPORT_STATS] == ((s.rows_end + 15) & ~(size_t)15));
                            for (int K : { 1, 4 }) {
                                size_t at = 0;
                                for (int c = 0; c < K; c++) {
                                    size_t b0 = 1, b1 = 0;
                                    deliver_chunk_bytes(rows, s.row_bytes, c, K, sec.end, &b0, &b1);
                                    CHECK(b0 == at && b1 >= b0 && b0 % s.row_bytes == 0);
                                    CHECK(c + 1 == K ? b1 == sec.end : (b1 % s.row_bytes == 0 && b1 <= s.rows_end));
                                    at = b1;
                                }
                                CHECK(at == sec.end);
                            }
                            /* a window's room holds any step of at most W blocks wherever it begins, sections included; so does a row's fixed pitch */
                            const size_t room = ((deliver_ratio_window_bytes(W, R, L, M, width, rows) + 15) & ~(size_t)15) + report_room(live, rows, W);
                            CHECK(sec.end <= room);
                            CHECK(s.pitch <= gdg_deliver_pitch(R, L, M, W * 8192) && gdg_deliver_pitch(R, L, M, W * 8192) % 4 == 0);
                            /* 1/1: the figures of the factor alone */
                            if (L == 1 && M == 1) {
                                const DeliverStep o = deliver_step(w, off, R, width, rows);
                                CHECK(s.samples == w * 8192 / (size_t)R && s.pitch == s.samples && s.copy_bytes == s.row_bytes);
                                CHECK(o.samples == s.samples && o.row_bytes == s.row_bytes && o.file_at == s.file_at && o.rows_end == s.rows_end);
                                CHECK(o.file_at == off / (size_t)R * width && o.row_bytes == w * 8192 * width / (size_t)R);
                                CHECK(deliver_ratio_window_bytes(W, R, 1, 1, width, rows) == deliver_window_bytes(W, R, width, rows));
                                CHECK(deliver_window_bytes(W, R, width, rows) == rows * (W * 8192 / (size_t)R) * width);
                                CHECK(s.first_out == (pos * 8192 + off) / (size_t)R);
                            }
                            cases++;
                        }
                        /* a slice writes what gdg_batch_out_samples says, and the slices' counts sum to the job's */
                        CHECK(file_end == (size_t)gdg_deliver_samples(R, L, M, pos * 8192, slice * 8192) * width);
                        delivered += gdg_deliver_samples(R, L, M, pos * 8192, slice * 8192);
                    }
                    CHECK(delivered == gdg_deliver_samples(R, L, M, 0, job * 8192));
                    CHECK(delivered == ceil_div((u64)job * 8192 / (u64)R * (u64)L, (u64)M));
                }
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("OK delivered ratio step bytes; %d step cases\n", cases);
    return 0;
}
