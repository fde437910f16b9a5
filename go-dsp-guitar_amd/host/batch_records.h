/*
 * batch_records.h -- the nine kinds of records a batch call keeps, stated once for the C++ twin: one table row per kind (element size,
 * shape, the words of its refusals, its getter of include/gdg.h behind one signature), one store per kind, and the paths every kind
 * shares: the size-then-fill fetch of a whole list, the fetch checked against the counts the engine expects with its rows filed to
 * the engine's (the four port kinds over shards), what Engine::LastBatch* and the gdgh_engine_last_batch_* wrappers hand out, and
 * the state a job without a block leaves.  Plain C++17 over include/gdg.h: no Engine and no HIP, so a stand-alone program can hold
 * it against stub getters (tests/native/batch_records_check.cpp).
 */
#ifndef GDG_BATCH_RECORDS_H
#define GDG_BATCH_RECORDS_H

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gdg.h"

namespace gdg {
namespace records {

using Error = std::string;          /* "" == nil, as in gdg_host.hpp */

/* in the order a one-shard engine asks its context for them */
enum Kind { REPORT = 0, TRUE_PEAK, ALIGN, SPECTRUM, FIT, GRAM, TRANSFER, DELIVERED, TAPFIT, KINDS };
enum Shape { PORTS_BLOCKS, PORTS_BLOCKS_BANDS, FITS_BLOCKS, BLOCKS_PER };

/* a kind's getter behind one signature: `rows` = ports or fits, `per` = the elements of one (row, block) or of one block.  The Gram
 * getter reports blocks alone: it takes the list's ports from *rows and gives P (P + 1) / 2 */
using Getter = int (*)(gdg_ctx *ctx, void *records, size_t capacity, int *rows, size_t *blocks, size_t *per);

inline int getReport(gdg_ctx *c, void *r, size_t cap, int *rows, size_t *blocks, size_t *) { return gdg_batch_report(c, static_cast<gdg_block_stats *>(r), cap, rows, blocks); }
inline int getTruePeak(gdg_ctx *c, void *r, size_t cap, int *rows, size_t *blocks, size_t *) { return gdg_batch_true_peak(c, static_cast<gdg_block_true_peak *>(r), cap, rows, blocks); }
inline int getAlign(gdg_ctx *c, void *r, size_t cap, int *rows, size_t *blocks, size_t *) { return gdg_batch_align(c, static_cast<gdg_block_align *>(r), cap, rows, blocks); }
inline int getSpectrum(gdg_ctx *c, void *r, size_t cap, int *rows, size_t *blocks, size_t *per) {
    int bands = (int)*per;
    const int rc = gdg_batch_spectrum(c, static_cast<double *>(r), cap, rows, blocks, &bands);
    *per = (size_t)bands;
    return rc;
}
inline int getFit(gdg_ctx *c, void *r, size_t cap, int *rows, size_t *blocks, size_t *) { return gdg_batch_fit(c, static_cast<gdg_block_fit *>(r), cap, rows, blocks); }
inline int getGram(gdg_ctx *c, void *r, size_t cap, int *rows, size_t *blocks, size_t *per) {
    *per = (size_t)*rows * ((size_t)*rows + 1) / 2;
    return gdg_batch_gram(c, static_cast<double *>(r), cap, blocks);
}
inline int getTransfer(gdg_ctx *c, void *r, size_t cap, int *, size_t *blocks, size_t *per) { return gdg_batch_transfer(c, static_cast<double *>(r), cap, blocks, per); }
inline int getDelivered(gdg_ctx *c, void *r, size_t cap, int *rows, size_t *blocks, size_t *) { return gdg_batch_out_records(c, static_cast<gdg_block_delivered *>(r), cap, rows, blocks); }
inline int getTapFit(gdg_ctx *c, void *r, size_t cap, int *, size_t *blocks, size_t *per) { return gdg_batch_tapfit(c, static_cast<double *>(r), cap, blocks, per); }

struct Row {
    size_t size;                    /* of an element: a record, or a double */
    Shape shape;
    bool ports;                     /* one of the four kinds an engine of any shard count keeps, filed row by row (the delivered rows' records have the shape, but one shard only) */
    const char *last, *kept, *setter, *room;      /* "<last>: the last batch call kept no <kept> (<setter> comes before the call)"; "... too little room for the <room>" */
    const char *what, *whatMaster;  /* a count mismatch names the records so, from a shard or the plain run and from the master's finish (the spectrum's text is its own) */
    Getter get;
};

constexpr Row table[KINDS] = {
    { sizeof(gdg_block_stats), PORTS_BLOCKS, true, "LastBatchReport", "report", "SetBatchReport", "records", "a report", "a master report", getReport },
    { sizeof(gdg_block_true_peak), PORTS_BLOCKS, true, "LastBatchTruePeak", "true-peak records", "SetBatchTruePeak", "records", "true-peak records", "true-peak records", getTruePeak },
    { sizeof(gdg_block_align), PORTS_BLOCKS, true, "LastBatchAlign", "alignment records", "SetBatchAlign", "records", "alignment records", "alignment records", getAlign },
    { sizeof(double), PORTS_BLOCKS_BANDS, true, "LastBatchSpectrum", "spectrum", "SetBatchSpectrum", "bands", nullptr, nullptr, getSpectrum },
    { sizeof(gdg_block_fit), FITS_BLOCKS, false, "LastBatchFit", "fit records", "SetBatchFits", "records", nullptr, nullptr, getFit },
    { sizeof(double), BLOCKS_PER, false, "LastBatchGram", "Gram records", "SetBatchGram", "records", nullptr, nullptr, getGram },
    { sizeof(double), BLOCKS_PER, false, "LastBatchTransfer", "transfer records", "SetBatchTransfers", "records", nullptr, nullptr, getTransfer },
    { sizeof(gdg_block_delivered), PORTS_BLOCKS, false, "LastBatchDelivered", "records of the delivered rows", "SetBatchDelivered", "records", nullptr, nullptr, getDelivered },
    { sizeof(double), BLOCKS_PER, false, "LastBatchTapFit", "tap-fit records", "SetBatchTapFits", "records", nullptr, nullptr, getTapFit },
};

/* the last batch call's records of one kind: `bytes` holds rows x blocks x per elements ([blocks][per] ones: blocks x per) */
struct RecordStore {
    std::vector<unsigned char> bytes;
    int rows = 0;
    size_t blocks = 0, per = 0;
    bool valid = false;
};

/* what the engine's settings say a job keeps of a kind */
struct Expect { bool on; int rows; size_t per; };

inline size_t elements(Kind k, int rows, size_t blocks, size_t per) { return (table[k].shape == BLOCKS_PER ? 1 : (size_t)rows) * blocks * per; }

/* a store of zero records at the expected counts: what a call over shards files its rows into */
inline void begin(Kind k, RecordStore &s, int rows, size_t blocks, size_t per) {
    s.rows = rows; s.blocks = blocks; s.per = per;
    s.bytes.assign(elements(k, rows, blocks, per) * table[k].size, 0);
}

/* size call, assign, fill call: the context's whole list is the store's.  `rows`: the Gram list's ports (see Getter) */
inline Error fetchWhole(Kind k, gdg_ctx *ctx, RecordStore &s, int rows = 0) {
    size_t blocks = 0, per = 1;
    if (table[k].get(ctx, nullptr, 0, &rows, &blocks, &per) != GDG_OK) return gdg_last_error(ctx);
    begin(k, s, rows, blocks, per);
    if (!s.bytes.empty() && table[k].get(ctx, s.bytes.data(), s.bytes.size() / table[k].size, &rows, &blocks, &per) != GDG_OK) return gdg_last_error(ctx);
    s.valid = true;
    return "";
}

/* a port kind's rows x blocks x per elements of a context's last call, checked against what the engine expects of that context */
inline Error fetchExpected(Kind k, gdg_ctx *ctx, RecordStore &s, int rows, size_t blocks, size_t per, bool master = false) {
    int p = 0;
    size_t nb = 0, b = per;
    begin(k, s, rows, blocks, per);
    if (table[k].get(ctx, s.bytes.data(), s.bytes.size() / table[k].size, &p, &nb, &b) != GDG_OK) return gdg_last_error(ctx);
    char buf[512];
    if (table[k].shape == PORTS_BLOCKS_BANDS) {
        if (p == rows && nb == blocks && b == per) return "";
        snprintf(buf, sizeof(buf), "a spectrum of %d ports x %zu blocks x %d bands where %d x %zu x %d were expected", p, nb, (int)b, rows, blocks, (int)per);
    } else {
        if (p == rows && nb == blocks) return "";
        snprintf(buf, sizeof(buf), "%s of %d ports x %zu blocks where %d x %zu were expected", master ? table[k].whatMaster : table[k].what, p, nb, rows, blocks);
    }
    return buf;
}

/* ... and filed into the engine's store `last`: the first `n0` rows the context gave to the rows from `to0` on (a shard's chain rows to
 * its channels, the finish's two to the master's), the `n1` rows behind them to the rows from `to1` on (shard 0's last to the metronome's) */
inline Error fileRows(Kind k, gdg_ctx *ctx, RecordStore &last, int rows, size_t to0, size_t n0, size_t to1, size_t n1, bool master = false) {
    RecordStore got;
    Error e = fetchExpected(k, ctx, got, rows, last.blocks, last.per, master);
    if (!e.empty()) return e;
    const size_t row = last.blocks * last.per * table[k].size;
    if (n0 && row) memcpy(&last.bytes[to0 * row], got.bytes.data(), n0 * row);
    if (n1 && row) memcpy(&last.bytes[to1 * row], &got.bytes[n0 * row], n1 * row);
    return "";
}

/* under Engine::LastBatch*: the refusal, or the store's elements and counts (any of the three may be NULL) */
template <class Per = size_t>
inline Error last(Kind k, const RecordStore &s, const void **data, size_t *n, int *rows, size_t *blocks, Per *per = nullptr) {
    if (!s.valid) return std::string(table[k].last) + ": the last batch call kept no " + table[k].kept + " (" + table[k].setter + " comes before the call)";
    if (data) *data = s.bytes.data();
    if (n) *n = s.bytes.size() / table[k].size;
    if (rows) *rows = s.rows;
    if (blocks) *blocks = s.blocks;
    if (per) *per = (Per)s.per;
    return "";
}

/* ... as a vector of the kind's element type */
template <class T, class Per = size_t>
inline Error lastAs(Kind k, const RecordStore &s, std::vector<T> &records, int *rows, size_t *blocks, Per *per = nullptr) {
    const void *data = nullptr;
    size_t n = 0;
    Error e = last(k, s, &data, &n, rows, blocks, per);
    if (!e.empty()) return e;
    records.resize(n);
    if (n) memcpy(records.data(), data, n * sizeof(T));
    return "";
}

/* under gdgh_engine_last_batch_*: the counts, then -- records != NULL -- the elements, when `capacity` of them have room */
template <class Per = size_t>
inline Error copyOut(Kind k, const RecordStore &s, void *records, size_t capacity, int *rows, size_t *blocks, Per *per = nullptr) {
    const void *data = nullptr;
    size_t n = 0;
    Error e = last(k, s, &data, &n, rows, blocks, per);
    if (!e.empty() || !records) return e;
    if (capacity < n) return std::string(table[k].last) + ": too little room for the " + table[k].room;
    if (n) memcpy(records, data, n * table[k].size);
    return "";
}

/* what a job without a block leaves: every kind in force is kept, as an empty list at the counts the settings give.  The delivered
 * rows' records stay invalid, as the reset in front of the call left them: the statement this loop replaced left that kind out.  The
 * omission is kept, not decided. */
inline void emptyJob(RecordStore (&stores)[KINDS], const Expect (&want)[KINDS]) {
    for (int k = 0; k < KINDS; k++) {
        if (k == DELIVERED) continue;
        stores[k].valid = want[k].on;
        if (!table[k].ports) begin((Kind)k, stores[k], want[k].rows, 0, want[k].per);      /* the port kinds were sized when the call began */
    }
}

}  // namespace records
}  // namespace gdg

#endif
