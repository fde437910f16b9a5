/*
 * batch_records_check.cpp -- the C++ twin's one table of the nine record kinds (host/batch_records.h) against stub getters, without
 * libgdg and without a GPU.  The stubs below are the nine gdg_batch_* getters over a context that is a plain struct: per kind the counts
 * it serves, a byte pattern of its own for the elements, and a switch that makes the getter fail with a text.  For all nine kinds: the
 * two-call protocol fills the store with the stub's values and counts; `last` before any fetch refuses with the text the nine
 * Engine::LastBatch* bodies carried (the literals below are theirs); copyOut with no destination gives the counts only, with too little
 * room it refuses with the kind's text, with room it gives the bytes; a failing getter's error is passed on.  For the four port kinds:
 * fileRows puts a shard's n chain rows at `first`, shard 0's extra row at N + 2 and the finish's two rows at N, and a count mismatch
 * refuses with the text of the engine's, the spectrum's three-number form included.  Last: emptyJob leaves every kind as the statement
 * it replaced in Engine::BatchRun left it -- the delivered rows' records untouched.  Built by tests/test_batch_records_host.py, plain and
 * under AddressSanitizer and UBSan.
 */
#include "batch_records.h"

#include <cstdio>
#include <initializer_list>
#include <string>

using namespace gdg::records;

struct Served { int rows; size_t blocks, per; bool fail; };
struct gdg_ctx { Served kind[KINDS]; std::string error; int calls[KINDS]; };

static unsigned char pattern(int kind, size_t i) { return (unsigned char)(1 + kind * 29 + i * 7 + (i >> 8)); }

/* what every stub does behind its own signature: the counts, then -- records != NULL -- `n` elements of the kind's pattern */
static int serve(gdg_ctx *ctx, int kind, void *records, size_t capacity, size_t n) {
    ctx->calls[kind]++;
    if (ctx->kind[kind].fail) { ctx->error = std::string("stub: the getter of ") + table[kind].last + " failed"; return GDG_ERR_INVALID; }
    if (!records) return GDG_OK;
    if (capacity < n) { ctx->error = "stub: too little capacity"; return GDG_ERR_INVALID; }
    for (size_t i = 0; i < n * table[kind].size; i++) static_cast<unsigned char *>(records)[i] = pattern(kind, i);
    return GDG_OK;
}

extern "C" {
const char *gdg_last_error(const gdg_ctx *ctx) { return ctx->error.c_str(); }
#define PORTS_GETTER(name, type, K)                                                                        \
    int name(gdg_ctx *ctx, type *records, size_t capacity, int *ports, size_t *blocks) {                  \
        const Served &s = ctx->kind[K];                                                                    \
        *ports = s.rows; *blocks = s.blocks;                                                               \
        return serve(ctx, K, records, capacity, (size_t)s.rows * s.blocks);                                \
    }
PORTS_GETTER(gdg_batch_report, gdg_block_stats, REPORT)
PORTS_GETTER(gdg_batch_true_peak, gdg_block_true_peak, TRUE_PEAK)
PORTS_GETTER(gdg_batch_align, gdg_block_align, ALIGN)
PORTS_GETTER(gdg_batch_fit, gdg_block_fit, FIT)
PORTS_GETTER(gdg_batch_out_records, gdg_block_delivered, DELIVERED)
int gdg_batch_spectrum(gdg_ctx *ctx, double *bands, size_t capacity, int *ports, size_t *blocks, int *n_bands) {
    const Served &s = ctx->kind[SPECTRUM];
    *ports = s.rows; *blocks = s.blocks; *n_bands = (int)s.per;
    return serve(ctx, SPECTRUM, bands, capacity, (size_t)s.rows * s.blocks * s.per);
}
int gdg_batch_gram(gdg_ctx *ctx, double *out, size_t capacity, size_t *blocks) {
    const Served &s = ctx->kind[GRAM];
    *blocks = s.blocks;
    return serve(ctx, GRAM, out, capacity, s.blocks * s.per);
}
#define BLOCKS_GETTER(name, K)                                                                             \
    int name(gdg_ctx *ctx, double *out, size_t capacity, size_t *blocks, size_t *doubles_per_block) {     \
        const Served &s = ctx->kind[K];                                                                    \
        *blocks = s.blocks; *doubles_per_block = s.per;                                                    \
        return serve(ctx, K, out, capacity, s.blocks * s.per);                                             \
    }
BLOCKS_GETTER(gdg_batch_transfer, TRANSFER)
BLOCKS_GETTER(gdg_batch_tapfit, TAPFIT)
}

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static bool holds(Kind k, const RecordStore &s, size_t from, size_t n, size_t pattern_from) {      /* n bytes of the kind's pattern */
    for (size_t i = 0; i < n; i++) if (s.bytes[from + i] != pattern(k, pattern_from + i)) return false;
    return true;
}
static bool zero(const RecordStore &s, size_t from, size_t n) {
    for (size_t i = 0; i < n; i++) if (s.bytes[from + i]) return false;
    return true;
}

/* the refusals of the nine Engine::LastBatch* bodies and of the nine gdgh_engine_last_batch_* wrappers, as they stood */
static const char *const kNone[KINDS] = {
    "LastBatchReport: the last batch call kept no report (SetBatchReport comes before the call)",
    "LastBatchTruePeak: the last batch call kept no true-peak records (SetBatchTruePeak comes before the call)",
    "LastBatchAlign: the last batch call kept no alignment records (SetBatchAlign comes before the call)",
    "LastBatchSpectrum: the last batch call kept no spectrum (SetBatchSpectrum comes before the call)",
    "LastBatchFit: the last batch call kept no fit records (SetBatchFits comes before the call)",
    "LastBatchGram: the last batch call kept no Gram records (SetBatchGram comes before the call)",
    "LastBatchTransfer: the last batch call kept no transfer records (SetBatchTransfers comes before the call)",
    "LastBatchDelivered: the last batch call kept no records of the delivered rows (SetBatchDelivered comes before the call)",
    "LastBatchTapFit: the last batch call kept no tap-fit records (SetBatchTapFits comes before the call)",
};
static const char *const kRoom[KINDS] = {
    "LastBatchReport: too little room for the records", "LastBatchTruePeak: too little room for the records", "LastBatchAlign: too little room for the records",
    "LastBatchSpectrum: too little room for the bands", "LastBatchFit: too little room for the records", "LastBatchGram: too little room for the records",
    "LastBatchTransfer: too little room for the records", "LastBatchDelivered: too little room for the records", "LastBatchTapFit: too little room for the records",
};

int main() {
    static_assert(REPORT == 0 && TRUE_PEAK == 1 && ALIGN == 2 && SPECTRUM == 3 && FIT == 4 && GRAM == 5 && TRANSFER == 6 && DELIVERED == 7 && TAPFIT == 8 && KINDS == 9, "the literals below are in this order");
    const size_t size[KINDS] = { sizeof(gdg_block_stats), sizeof(gdg_block_true_peak), sizeof(gdg_block_align), 8, sizeof(gdg_block_fit), 8, 8, sizeof(gdg_block_delivered), 8 };
    const int N = 5, first = 2, n = 2;                     /* a job of 5 channels; the shard under test holds channels 2 and 3 */
    const size_t blocks = 3, bands = 4;
    int cases = 0;
    gdg_ctx ctx = {};
    /* the plain run's context: N + 3 + 1 ports (one blend), 2 fits, a Gram list of 3 ports, 21 tap-fit doubles, 2 transfer pairs in groups of 32 */
    ctx.kind[REPORT] = ctx.kind[TRUE_PEAK] = ctx.kind[ALIGN] = ctx.kind[DELIVERED] = { N + 4, blocks, 1, false };
    ctx.kind[SPECTRUM] = { N + 4, blocks, bands, false };
    ctx.kind[FIT] = { 2, blocks, 1, false };
    ctx.kind[GRAM] = { 3, blocks, 6, false };
    ctx.kind[TAPFIT] = { 0, blocks, 21, false };
    ctx.kind[TRANSFER] = { 0, blocks, 2 * (4096 / 32 + 1) * 4, false };
    RecordStore stores[KINDS];
    for (int i = 0; i < KINDS; i++) {
        const Kind k = (Kind)i;
        const Served &want = ctx.kind[k];
        RecordStore &s = stores[k];
        CHECK(table[k].size == size[k]);
        const size_t count = elements(k, want.rows, want.blocks, want.per);
        CHECK(count == (table[k].shape == BLOCKS_PER ? want.blocks * want.per : (size_t)want.rows * want.blocks * want.per));
        /* before any fetch: the kind's refusal, from `last` and through copyOut, and nothing written */
        int rows = -1;
        size_t nb = 77, per = 77;
        CHECK(last(k, s, nullptr, nullptr, &rows, &nb, &per) == kNone[k] && copyOut(k, s, nullptr, 0, &rows, &nb, &per) == kNone[k]);
        CHECK(rows == -1 && nb == 77 && per == 77);
        /* a getter that fails passes the context's error through, and the store stays invalid */
        ctx.kind[k].fail = true;
        CHECK(fetchWhole(k, &ctx, s, want.rows) == std::string("stub: the getter of ") + table[k].last + " failed" && !s.valid);
        if (table[k].ports) CHECK(fetchExpected(k, &ctx, s, want.rows, want.blocks, want.per) == std::string("stub: the getter of ") + table[k].last + " failed" && !s.valid);
        ctx.kind[k].fail = false;
        /* size call, assign, fill call */
        ctx.calls[k] = 0;
        CHECK(fetchWhole(k, &ctx, s, want.rows).empty() && ctx.calls[k] == 2 && s.valid);
        CHECK(s.blocks == want.blocks && s.per == want.per && s.rows == want.rows);
        CHECK(s.bytes.size() == count * size[k] && holds(k, s, 0, s.bytes.size(), 0));
        /* last: the elements and the counts, `per` as an int too (the spectrum's band count) */
        const void *data = nullptr;
        size_t elems = 0;
        int per_int = -1;
        CHECK(last(k, s, &data, &elems, &rows, &nb, &per).empty() && data == s.bytes.data() && elems == count && rows == s.rows && nb == blocks && per == want.per);
        CHECK(last(k, s, nullptr, nullptr, nullptr, nullptr, &per_int).empty() && per_int == (int)want.per);
        /* copyOut: no destination -- the counts only; too little room -- the kind's refusal behind the counts; room -- the bytes */
        std::vector<unsigned char> out(count * size[k] + 1, 0xEE);
        rows = -1; nb = 77; per = 77;
        CHECK(copyOut(k, s, nullptr, 0, &rows, &nb, &per).empty() && rows == s.rows && nb == blocks && per == want.per);
        rows = -1; nb = 77;
        CHECK(copyOut(k, s, out.data(), count - 1, &rows, &nb).compare(kRoom[k]) == 0 && rows == s.rows && nb == blocks && out[0] == 0xEE);
        CHECK(copyOut(k, s, out.data(), count, nullptr, nullptr).empty() && memcmp(out.data(), s.bytes.data(), count * size[k]) == 0 && out[count * size[k]] == 0xEE);
        cases++;
    }
    {   /* lastAs in the kind's own element type */
        std::vector<gdg_block_fit> fit;
        int fits = 0;
        size_t nb = 0;
        CHECK(lastAs(FIT, stores[FIT], fit, &fits, &nb).empty() && fits == 2 && nb == blocks && fit.size() == 2 * blocks && memcmp(fit.data(), stores[FIT].bytes.data(), stores[FIT].bytes.size()) == 0);
        std::vector<double> sp;
        int ports = 0, nbands = 0;
        CHECK(lastAs(SPECTRUM, stores[SPECTRUM], sp, &ports, &nb, &nbands).empty() && ports == N + 4 && nbands == (int)bands && sp.size() == (size_t)(N + 4) * blocks * bands);
        cases++;
    }
    /* a list without a block: fetchWhole makes one call and keeps an empty, valid list at the getter's counts */
    {
        RecordStore s;
        ctx.kind[FIT] = { 2, 0, 1, false };
        ctx.calls[FIT] = 0;
        CHECK(fetchWhole(FIT, &ctx, s).empty() && ctx.calls[FIT] == 1 && s.valid && s.bytes.empty() && s.rows == 2 && s.blocks == 0);
        cases++;
    }
    /* ---- the four port kinds over shards: the engine's store of N + 3 rows; a shard of n chain rows and, on shard 0, the metronome's; the finish's two */
    for (Kind k : { REPORT, TRUE_PEAK, ALIGN, SPECTRUM }) {
        const size_t per = k == SPECTRUM ? bands : 1, row = blocks * per * size[k];
        RecordStore engine;
        begin(k, engine, N + 3, blocks, per);
        CHECK(engine.bytes.size() == (size_t)(N + 3) * row && zero(engine, 0, engine.bytes.size()) && !engine.valid);
        /* a later shard: its n chain rows at `first`, its metronome row (silent there) nowhere */
        ctx.kind[k] = { n + 1, blocks, per, false };
        CHECK(fileRows(k, &ctx, engine, n + 1, first, n, N + 2, 0).empty());
        CHECK(zero(engine, 0, first * row) && holds(k, engine, first * row, n * row, 0) && zero(engine, (first + n) * row, (N + 3 - first - n) * row));
        /* shard 0 (here: channels 0 and 1): its extra row goes to N + 2 */
        CHECK(fileRows(k, &ctx, engine, n + 1, 0, n, N + 2, 1).empty());
        CHECK(holds(k, engine, 0, n * row, 0) && holds(k, engine, (size_t)(N + 2) * row, row, n * row) && zero(engine, (size_t)N * row, 2 * row));
        /* the finish: two rows to N */
        ctx.kind[k] = { 2, blocks, per, false };
        CHECK(fileRows(k, &ctx, engine, 2, N, 2, 0, 0, /*master=*/true).empty());
        CHECK(holds(k, engine, (size_t)N * row, 2 * row, 0) && holds(k, engine, (size_t)(N + 2) * row, row, n * row) && holds(k, engine, first * row, n * row, 0));
        CHECK(zero(engine, (size_t)(first + n) * row, (size_t)(N - first - n) * row));      /* channel 4: no shard filed it */
        /* a count mismatch (fewer than asked for, so that the stub has room to serve them): the engine's texts */
        ctx.kind[k] = { 2, blocks - 1, per - (k == SPECTRUM ? 1 : 0), false };
        char want[256], master[256];
        if (k == SPECTRUM) {
            snprintf(want, sizeof(want), "a spectrum of 2 ports x %zu blocks x %d bands where 3 x %zu x %d were expected", blocks - 1, (int)bands - 1, blocks, (int)bands);
            snprintf(master, sizeof(master), "%s", want);
        } else {
            const char *what = k == REPORT ? "a report" : k == ALIGN ? "alignment records" : "true-peak records";
            snprintf(want, sizeof(want), "%s of 2 ports x %zu blocks where 3 x %zu were expected", what, blocks - 1, blocks);
            snprintf(master, sizeof(master), "%s of 2 ports x %zu blocks where 3 x %zu were expected", k == REPORT ? "a master report" : what, blocks - 1, blocks);
        }
        const std::vector<unsigned char> before = engine.bytes;
        CHECK(fileRows(k, &ctx, engine, n + 1, first, n, N + 2, 1) == want && fileRows(k, &ctx, engine, 3, N, 2, 0, 0, true) == master && engine.bytes == before);
        RecordStore plain;
        CHECK(fetchExpected(k, &ctx, plain, 3, blocks, per) == want && !plain.valid);
        cases++;
    }
    /* ---- a job without a block.  THE STATEMENT emptyJob REPLACED, restated: transfer, tap fit, Gram and fit -- valid = the kind is on, no
     * block, the list cleared, the counts from the settings (doubles per block; the Gram list's ports); report, spectrum, alignment and
     * true peak -- valid = the kind is on, nothing else; the delivered rows' records -- not named, so whatever the reset left */
    for (int mask = 0; mask < (1 << KINDS); mask += 7) {
        RecordStore job[KINDS];
        Expect want[KINDS];
        for (int k = 0; k < KINDS; k++) {
            const bool on = (mask >> k) & 1;
            want[k] = { on, k == FIT ? 2 : k == GRAM ? 3 : N + 3, k == GRAM ? (size_t)6 : k == TAPFIT ? (size_t)(on ? 21 : 0) : k == TRANSFER ? (size_t)1032 : k == SPECTRUM ? bands : (size_t)1 };
            /* what the last call and the reset in front of this one left: old records, invalid; the port kinds that are on sized for no block */
            job[k].bytes.assign(5 * table[k].size, 0x5A);
            job[k].rows = 9; job[k].blocks = 5; job[k].per = 1; job[k].valid = false;
            if (table[k].ports && on) begin((Kind)k, job[k], N + 3, 0, want[k].per);
        }
        emptyJob(job, want);
        for (int k = 0; k < KINDS; k++) {
            const bool on = (mask >> k) & 1;
            if (k == DELIVERED) { CHECK(!job[k].valid && job[k].rows == 9 && job[k].blocks == 5 && job[k].bytes.size() == 5 * table[k].size); continue; }
            CHECK(job[k].valid == on);
            if (table[k].ports) { CHECK(on ? job[k].bytes.empty() && job[k].rows == N + 3 && job[k].blocks == 0 : job[k].rows == 9 && job[k].blocks == 5 && job[k].bytes.size() == 5 * table[k].size); continue; }
            CHECK(job[k].bytes.empty() && job[k].blocks == 0 && job[k].per == want[k].per && job[k].rows == want[k].rows);
            /* ... and what LastBatch* then hands out: the refusal of a kind that is off, no element and the settings' counts of one that is on */
            int rows = -1;
            size_t nb = 77, per = 77, elems = 77;
            if (!on) CHECK(last((Kind)k, job[k], nullptr, &elems, &rows, &nb, &per) == kNone[k]);
            else CHECK(last((Kind)k, job[k], nullptr, &elems, &rows, &nb, &per).empty() && elems == 0 && nb == 0 && per == want[k].per && rows == want[k].rows);
        }
        cases++;
    }
    if (failures) return 1;
    printf("OK %d cases over %d kinds\n", cases, (int)KINDS);
    return 0;
}
