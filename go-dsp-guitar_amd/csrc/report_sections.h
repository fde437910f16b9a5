/*
 * report_sections.h -- where the render report's record kinds ride in a batch call's download half: the ONE statement of that layout.
 * A step (or a master finish's piece) sends its encoded rows down; behind them follows one section per live kind, in this fixed order:
 * block statistics, band spectrum, alignment records, true-peak records.  A section is [rows][w] elements -- `rows` record rows (N + 3 for
 * a plain call, N + 1 for a shard, 2 for a finish), `w` blocks -- of the kind's element size per port and block.  The block loop starts
 * every live section at the next 16 bytes behind whatever precedes it; the finish packs them.  Behind the kinds' sections a step of the
 * block loop sends the five list records' (LIST_KINDS below), by the same 16-byte rule.  Pure host arithmetic: no HIP header is needed to
 * compile this file (tests/native/report_sections_check.cpp and list_chain_check.cpp hold it against the formulas it replaced).
 */
#ifndef GDG_REPORT_SECTIONS_H
#define GDG_REPORT_SECTIONS_H

#include <stddef.h>
#include <string.h>

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

/* The list records are no further kinds: their rows are a call's own lists, not its ports.  ONE RULE for all five: a step of the block loop
 * sends them down behind the last live kind's section -- behind its rows when no kind is live -- in the order of this enum, each as [rows][w]
 * elements of `elem` bytes from the next 16 bytes behind whatever precedes it; a list that is off takes no byte and moves nothing.  The
 * finish calls never carry them.  (rows, elem) per kind (include/gdg.h: FIT, GRAM, TAPFIT, TRANSFER, DELIVERED RECORDS):
 *   LIST_FIT        (fits, 368)                            the blend fits' records
 *   LIST_GRAM       (1, P (P + 1) / 2 doubles)             the Gram list of P ports
 *   LIST_TAPFIT     (1, D doubles)                         the tap fits, D the list's sum of V (V + 1) / 2
 *   LIST_TRANSFER   (1, n_pairs (4096 / D + 1) 4 doubles)  the transfer records of n_pairs pairs in groups of D bins
 *   LIST_DELIVERED  (ports, 40)                            the records of the delivered rows */
enum { LIST_FIT, LIST_GRAM, LIST_TAPFIT, LIST_TRANSFER, LIST_DELIVERED, LIST_KINDS };
enum { FIT_RECORD_BYTES = 368 };
static inline size_t gram_record_bytes(size_t ports) { return ports * (ports + 1) / 2 * 8; }
static inline size_t transfer_record_bytes(size_t pairs, size_t group) { return pairs && group ? pairs * (4096 / group + 1) * 4 * 8 : 0; }
enum { DELIVERED_RECORD_BYTES = 40 };

/* what a list in force sends down per block: `rows` rows of one element of `elem` bytes; elem == 0 = the kind is off */
struct ListShape {
    size_t rows, elem;
    bool on() const { return elem != 0; }
};

/* a list's section behind `end` (at = end = `end` and no byte for a list that is off) ... */
struct ListSection { size_t at, bytes, end; };

static inline ListSection list_section(size_t end, const ListShape &shape, size_t w) {
    ListSection s = { end, 0, end };
    if (!shape.on()) return s;
    s.at = (end + 15) & ~(size_t)15;
    s.bytes = shape.rows * w * shape.elem;
    s.end = s.at + s.bytes;
    return s;
}

/* ... and what a half holds for it for a window of W blocks */
static inline size_t list_room(const ListShape &shape, size_t W) { return shape.on() ? 16 + shape.rows * W * shape.elem : 0; }

/* the five sections of a step, chained behind ReportSections::end; `end` is the end of what the step sends down */
struct ListSections { ListSection of[LIST_KINDS]; size_t end; };

static inline ListSections list_sections(size_t end, const ListShape *shape, size_t w) {
    ListSections s;
    for (int k = 0; k < LIST_KINDS; k++) end = (s.of[k] = list_section(end, shape[k], w)).end;
    s.end = end;
    return s;
}

/* ... and what a half holds for the chain for a window of W blocks, beside report_room */
static inline size_t lists_room(const ListShape *shape, size_t W) {
    size_t room = 0;
    for (int k = 0; k < LIST_KINDS; k++) room += list_room(shape[k], W);
    return room;
}

/* Filing a section that has come down: [rows][w] elements into a store of [rows][blocks], under the blocks from b0 on. */
static inline void list_file_rows(unsigned char *store, size_t blocks, const ListShape &shape, const unsigned char *section, size_t w, size_t b0) {
    for (size_t r = 0; r < shape.rows; r++) memcpy(store + (r * blocks + b0) * shape.elem, section + r * w * shape.elem, w * shape.elem);
}

#endif
