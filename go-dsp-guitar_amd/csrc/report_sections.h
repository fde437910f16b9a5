/*
 * report_sections.h -- where the render report's record kinds ride in a batch call's download half: the ONE statement of that layout.
 * A step (or a master finish's piece) sends its encoded rows down; behind them follows one section per live kind, in this fixed order:
 * block statistics, band spectrum, alignment records, true-peak records.  A section is [rows][w] elements -- `rows` record rows (N + 3 for
 * a plain call, N + 1 for a shard, 2 for a finish), `w` blocks -- of the kind's element size per port and block.  The block loop starts
 * every live section at the next 16 bytes behind whatever precedes it; the finish packs them.  Pure host arithmetic: no HIP header is
 * needed to compile this file (tests/native/report_sections_check.cpp holds it against the formulas it replaced).
 */
#ifndef GDG_REPORT_SECTIONS_H
#define GDG_REPORT_SECTIONS_H

#include <stddef.h>

enum { REPORT_STATS, REPORT_BANDS, REPORT_ALIGN, REPORT_TRUE_PEAK, REPORT_KINDS };

/* bytes per port and block: a gdg_block_stats (32), n_bands doubles, a gdg_block_align (40), a gdg_block_true_peak (16) */
static inline size_t report_elem(int kind, size_t n_bands) {
    return kind == REPORT_STATS ? 32 : kind == REPORT_BANDS ? n_bands * 8 : kind == REPORT_ALIGN ? 40 : 16;
}

/* the kinds a call collects: elem[k] = the kind's element size, 0 = the kind is off */
struct ReportLive {
    size_t elem[REPORT_KINDS];
    bool on(int k) const { return elem[k] != 0; }
    bool any() const { for (int k = 0; k < REPORT_KINDS; k++) if (elem[k]) return true; return false; }
};

/* every live kind's section (at, bytes; both 0 for a kind that is off) and the end of the last one (= base when none is live) */
struct ReportSections { size_t at[REPORT_KINDS], bytes[REPORT_KINDS], end; };

static inline ReportSections report_sections(const ReportLive &live, size_t rows, size_t w, size_t base, bool align16) {
    ReportSections s = { { 0, 0, 0, 0 }, { 0, 0, 0, 0 }, base };
    for (int k = 0; k < REPORT_KINDS; k++) {
        if (!live.on(k)) continue;
        s.at[k] = align16 ? (s.end + 15) & ~(size_t)15 : s.end;
        s.bytes[k] = rows * w * live.elem[k];
        s.end = s.at[k] + s.bytes[k];
    }
    return s;
}

/* what a half holds beside its rows for a window of W blocks: every live section and the 16 bytes its start may be moved by */
static inline size_t report_room(const ReportLive &live, size_t rows, size_t W) {
    size_t room = 0;
    for (int k = 0; k < REPORT_KINDS; k++) if (live.on(k)) room += 16 + rows * W * live.elem[k];
    return room;
}

/* The blend fit's records (include/gdg.h, FIT) are no fifth kind: their rows are the call's fits, not its ports.  A step of the block loop
 * sends them down behind the last live kind's section -- behind its rows when no kind is live -- from the next 16 bytes on: [fits][w]
 * records of 368 bytes.  No fit: no byte (at = end = `end`).  The finish calls never carry them. */
enum { FIT_RECORD_BYTES = 368 };
struct FitSection { size_t at, bytes, end; };

static inline FitSection fit_section(size_t end, size_t fits, size_t w) {
    FitSection s = { end, 0, end };
    if (!fits) return s;
    s.at = (end + 15) & ~(size_t)15;
    s.bytes = fits * w * FIT_RECORD_BYTES;
    s.end = s.at + s.bytes;
    return s;
}

/* ... and what a half holds for them for a window of W blocks, beside report_room */
static inline size_t fit_room(size_t fits, size_t W) { return fits ? 16 + fits * W * FIT_RECORD_BYTES : 0; }

/* The Gram records (include/gdg.h, GRAM) ride behind the fit section -- behind whatever precedes it when there is none -- from the next 16
 * bytes on: [w] records of P (P + 1) / 2 doubles for a list of P ports.  No list: no byte.  The finish calls never carry them. */
struct GramSection { size_t at, bytes, end; };

static inline size_t gram_record_bytes(size_t ports) { return ports * (ports + 1) / 2 * 8; }

static inline GramSection gram_section(size_t end, size_t ports, size_t w) {
    GramSection s = { end, 0, end };
    if (!ports) return s;
    s.at = (end + 15) & ~(size_t)15;
    s.bytes = w * gram_record_bytes(ports);
    s.end = s.at + s.bytes;
    return s;
}

/* ... and what a half holds for them for a window of W blocks */
static inline size_t gram_room(size_t ports, size_t W) { return ports ? 16 + W * gram_record_bytes(ports) : 0; }

/* The tap-fit records (include/gdg.h, TAPFIT) ride behind the Gram section -- behind whatever precedes it when there is none -- from the next
 * 16 bytes on: [w] records of D doubles, D the list's sum of V (V + 1) / 2.  No list: no byte.  The finish calls never carry them. */
struct TapFitSection { size_t at, bytes, end; };

static inline TapFitSection tapfit_section(size_t end, size_t doubles, size_t w) {
    TapFitSection s = { end, 0, end };
    if (!doubles) return s;
    s.at = (end + 15) & ~(size_t)15;
    s.bytes = w * doubles * 8;
    s.end = s.at + s.bytes;
    return s;
}

/* ... and what a half holds for them for a window of W blocks */
static inline size_t tapfit_room(size_t doubles, size_t W) { return doubles ? 16 + W * doubles * 8 : 0; }

#endif
