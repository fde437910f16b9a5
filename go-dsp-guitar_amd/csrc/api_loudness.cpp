/*
 * api_loudness.cpp -- the loudness records (include/gdg.h, LOUDNESS): the stand-alone calls, the batch switch and its getter,
 * what the slice runner calls (ctx.h), the refusals in the feature's own words, and the two planners (loudness.h) behind the C-ABI.
 * Part of the host side of libgdg.so (see ctx.h for the map).  The kernel is loudness.hip's.
 */
#include "ctx.h"

static_assert(GDG_LOUDNESS_STATE_DOUBLES == LOUDNESS_STATE && GDG_LOUDNESS_TILE == LOUDNESS_TILE, "include/gdg.h states the state's doubles and the tile");

/* ---- pure host arithmetic: no context; what is refused is kept per thread for gdg_last_error(NULL) ------------------------------------- */
int gdg_loudness_coefficients(uint32_t rate, double *out) {
    if (!out || !gdg_loudness_rate_ok(rate)) {
        char msg[160];
        snprintf(msg, sizeof msg, "loudness coefficients: rate %u, out %s; a multiple of 10 from 8000 on", rate, out ? "given" : "NULL");
        set_free_error(msg);
        return GDG_ERR_INVALID;
    }
    gdg_loudness_coefficients_at((double)rate, out);
    return GDG_OK;
}

size_t gdg_loudness_hops(uint32_t rate, size_t first, size_t count) {
    return gdg_loudness_rate_ok(rate) ? (size_t)gdg_loudness_hops_in(rate, first, count) : 0;
}

static int plan_refused(const char *what, int rc, uint32_t rate, long long bad, double target, double ceiling) {
    char msg[200];
    switch (rc) {
    case GDG_LOUDNESS_PLAN_RATE: snprintf(msg, sizeof msg, "%s: rate %u; a multiple of 10 from 8000 on", what, rate); break;
    case GDG_LOUDNESS_PLAN_PORT: snprintf(msg, sizeof msg, "%s: entry %lld names a port the records do not have", what, bad); break;
    case GDG_LOUDNESS_PLAN_WEIGHT: snprintf(msg, sizeof msg, "%s: weight %lld is negative or not finite", what, bad); break;
    case GDG_LOUDNESS_PLAN_RECORD: snprintf(msg, sizeof msg, "%s: hop record %lld is negative or not finite", what, bad); break;
    case GDG_LOUDNESS_PLAN_TARGET: snprintf(msg, sizeof msg, "%s: target_lufs = %g; finite", what, target); break;
    case GDG_LOUDNESS_PLAN_CEILING: snprintf(msg, sizeof msg, "%s: ceiling_dbtp = %g; finite", what, ceiling); break;
    case GDG_LOUDNESS_PLAN_PEAK: snprintf(msg, sizeof msg, "%s: port %lld has a NaN true_peak", what, bad); break;
    default: snprintf(msg, sizeof msg, "%s: at least one port, its records and somewhere to put the result", what); break;
    }
    set_free_error(msg);
    return GDG_ERR_INVALID;
}

int gdg_loudness_from_hops(const double *records, int n_ports, size_t n_hops, uint32_t rate, const int *port, const double *weight, int n, double *integrated,
                           double *momentary_max, double *short_term_max) {
    long long bad = -1;
    const int rc = gdg_loudness_plan(records, n_ports, n_hops, rate, port, weight, n, integrated, momentary_max, short_term_max, &bad);
    return rc == GDG_LOUDNESS_PLAN_OK ? GDG_OK : plan_refused("loudness from hops", rc, rate, bad, 0.0, 0.0);
}

int gdg_trim_from_loudness(const double *records, int n_ports, size_t n_hops, uint32_t rate, double target_lufs, double ceiling_dbtp, const gdg_block_true_peak *true_peak,
                           size_t blocks, double *gain, int *capped) {
    static_assert(sizeof(gdg_block_true_peak) == 2 * sizeof(double) && offsetof(gdg_block_true_peak, true_peak) == 0, "the planner strides over true_peak in doubles");
    long long bad = -1;
    const int rc = gdg_loudness_trim_plan(records, n_ports, n_hops, rate, target_lufs, ceiling_dbtp, reinterpret_cast<const double *>(true_peak), blocks, gain, capped, &bad);
    return rc == GDG_LOUDNESS_PLAN_OK ? GDG_OK : plan_refused("trim from loudness", rc, rate, bad, target_lufs, ceiling_dbtp);
}

/* ---- the stand-alone calls ------------------------------------------------------------------------------------------------------------ */
static int rows_check(gdg_ctx *ctx, int n_rows, size_t first, size_t count, uint32_t rate, bool continues, size_t room, size_t *hops) {
    if (n_rows <= 0) return fail(ctx, GDG_ERR_INVALID, "loudness rows: %d rows (at least 1)", n_rows);
    if (!gdg_loudness_rate_ok(rate)) return fail(ctx, GDG_ERR_INVALID, "loudness rows: rate %u; a hop is a tenth of a second in whole samples: a multiple of 10 from 8000 on", rate);
    if (!continues && first != 0) return fail(ctx, GDG_ERR_INVALID, "loudness rows: no state comes in, so a stream starts here, and it starts at sample 0, not %zu", first);
    if (first % LOUDNESS_TILE) return fail(ctx, GDG_ERR_INVALID, "loudness rows: a continuing call begins at a multiple of %d samples, not at %zu", LOUDNESS_TILE, first);
    *hops = (size_t)gdg_loudness_hops_in(rate, first, count);
    if (room < *hops) return fail(ctx, GDG_ERR_INVALID, "loudness rows: room for %zu hops per row, the samples %zu to %zu complete %zu", room, first, first + count, *hops);
    return GDG_OK;
}

int gdg_loudness_rows_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t first, size_t count, uint32_t rate, const double *d_state_in,
                             double *d_state_out, double *d_records, size_t records_stride) {
    if (!ctx) return GDG_ERR_INVALID;
    size_t hops = 0;
    const int rc = rows_check(ctx, n_rows, first, count, rate, d_state_in != nullptr, records_stride, &hops);
    if (rc != GDG_OK) return rc;
    if (count == 0) return GDG_OK;
    if (!d_rows || (hops && !d_records)) return fail(ctx, GDG_ERR_INVALID, "loudness rows: %s is NULL", !d_rows ? "the rows' pointer" : "the records' pointer");
    if (row_stride < count) return fail(ctx, GDG_ERR_INVALID, "loudness rows: a row stride of %zu samples for rows of %zu", row_stride, count);
    if (((uintptr_t)d_rows & 7) || ((uintptr_t)d_records & 7) || ((uintptr_t)d_state_in & 7) || ((uintptr_t)d_state_out & 7))
        return fail(ctx, GDG_ERR_INVALID, "loudness rows: rows, states and records are 8-byte aligned");
    enter_keep_fir_sums(ctx);
    gdg_ctx::Loudness &L = ctx->loud;
    const size_t state_bytes = (size_t)n_rows * LOUDNESS_STATE * sizeof(double);
    double *d_state = d_state_out;
    if (!d_state) {                                                          /* nowhere to leave the state: it lives in a buffer of the context for the launch */
        if (state_bytes > L.own_cap) {
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            hipFree(L.d_own);
            L.d_own = nullptr;
            L.own_cap = 0;
            if (hipMalloc((void **)&L.d_own, state_bytes) != hipSuccess) return fail(ctx, GDG_ERR_NOMEM, "loudness rows: cannot allocate the state of %d rows on the device", n_rows);
            L.own_cap = state_bytes;
        }
        d_state = L.d_own;
    }
    if (!d_state_in) HIP_TRY(ctx, hipMemsetAsync(d_state, 0, state_bytes, ctx->stream));
    else if (d_state_in != d_state) HIP_TRY(ctx, hipMemcpyAsync(d_state, d_state_in, state_bytes, hipMemcpyDeviceToDevice, ctx->stream));
    /* no hop completes: the kernel still moves the state on; it writes no record, and is given the state's buffer for the pointer it never uses */
    const gdg_loudness_params par = gdg_loudness_params_at(rate);
    ProfScope ps(ctx, GDG_K_WAVE);
    HIP_TRY(ctx, gdg_launch_block_loudness(d_rows, row_stride, (unsigned)n_rows, first, count, rate, first / gdg_loudness_hop(rate), hops ? records_stride : 0,
                                           par, d_state, hops ? d_records : d_state, ctx->stream));
    return GDG_OK;
}

int gdg_loudness_rows(gdg_ctx *ctx, const double *rows, size_t row_stride, int n_rows, size_t first, size_t count, uint32_t rate, const double *state_in, double *state_out,
                      double *records, size_t capacity) {
    if (!ctx) return GDG_ERR_INVALID;
    size_t hops = 0;
    int rc = rows_check(ctx, n_rows, first, count, rate, state_in != nullptr, capacity, &hops);
    if (rc != GDG_OK) return rc;
    if (count == 0) {
        if (state_out && state_in && state_out != state_in) memcpy(state_out, state_in, (size_t)n_rows * LOUDNESS_STATE * sizeof(double));
        if (state_out && !state_in) memset(state_out, 0, (size_t)n_rows * LOUDNESS_STATE * sizeof(double));
        return GDG_OK;
    }
    if (!rows || (hops && !records)) return fail(ctx, GDG_ERR_INVALID, "loudness rows: %s is NULL", !rows ? "the rows' pointer" : "the records' pointer");
    if (row_stride < count) return fail(ctx, GDG_ERR_INVALID, "loudness rows: a row stride of %zu samples for rows of %zu", row_stride, count);
    if (state_in)
        for (int r = 0; r < n_rows; r++)
            if (state_in[(size_t)r * LOUDNESS_STATE + 6] != (double)first)
                return fail(ctx, GDG_ERR_INVALID, "loudness rows: row %d's state stands at sample %.0f, this call begins at %zu", r, state_in[(size_t)r * LOUDNESS_STATE + 6], first);
    enter_keep_fir_sums(ctx);
    /* rows up compact into d_io[1] with the state behind them, records down from d_io[0] */
    const size_t rows_bytes = ((size_t)n_rows * count * sizeof(double) + 15) & ~(size_t)15, state_bytes = (size_t)n_rows * LOUDNESS_STATE * sizeof(double);
    rc = ensure_io(ctx, 1, rows_bytes + state_bytes);
    if (rc == GDG_OK) rc = ensure_io(ctx, 0, ((size_t)n_rows * hops + 2) * sizeof(double));
    if (rc != GDG_OK) return rc;
    double *d_rows = static_cast<double *>(ctx->d_io[1]), *d_records = static_cast<double *>(ctx->d_io[0]);
    double *d_state = reinterpret_cast<double *>(static_cast<unsigned char *>(ctx->d_io[1]) + rows_bytes);
    HIP_TRY(ctx, hipMemcpy2DAsync(d_rows, count * sizeof(double), rows, row_stride * sizeof(double), count * sizeof(double), (size_t)n_rows, hipMemcpyHostToDevice, ctx->stream));
    if (state_in) HIP_TRY(ctx, hipMemcpyAsync(d_state, state_in, state_bytes, hipMemcpyHostToDevice, ctx->stream));
    rc = gdg_loudness_rows_device(ctx, d_rows, count, n_rows, first, count, rate, state_in ? d_state : nullptr, d_state, d_records, hops);
    if (rc != GDG_OK) return rc;
    if (hops) HIP_TRY(ctx, hipMemcpy2DAsync(records, capacity * sizeof(double), d_records, hops * sizeof(double), hops * sizeof(double), (size_t)n_rows, hipMemcpyDeviceToHost, ctx->stream));
    if (state_out) HIP_TRY(ctx, hipMemcpyAsync(state_out, d_state, state_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return check_device_error(ctx);
}

/* ---- the batch calls' side --------------------------------------------------------------------------------------------------------------- */
int loudness_refused(gdg_ctx *ctx, const char *what, const char *why) {
    if (!ctx || !ctx->loud.on) return GDG_OK;
    return fail(ctx, GDG_ERR_UNSUPPORTED, "%s: the loudness records are on on this context (gdg_batch_loudness_enable); %s", what, why);
}

static void drop(double **d, size_t *cap) {
    hipFree(*d);
    *d = nullptr;
    *cap = 0;
}

void loudness_release(gdg_ctx *ctx) {
    gdg_ctx::Loudness &L = ctx->loud;
    drop(&L.d_state, &L.state_cap);
    drop(&L.d_records, &L.records_cap);
    drop(&L.d_own, &L.own_cap);
    L.valid = L.live = false;
}

size_t loudness_device_bytes(const gdg_ctx *ctx) { return ctx->loud.state_cap + ctx->loud.records_cap; }

int gdg_batch_loudness_enable(gdg_ctx *ctx, int enable) {
    if (!ctx) return GDG_ERR_INVALID;
    if (ctx->bstream.open)
        return fail(ctx, GDG_ERR_INVALID, "gdg_batch_loudness_enable: a streamed batch run is open on this context; the loudness records stay %s until gdg_batch_stream_close",
                    ctx->loud.on ? "on" : "off");
    const bool on = enable != 0;
    if (on == ctx->loud.on) return GDG_OK;
    enter(ctx, /*read_only=*/true);                                          /* configuration: no state of the context changes */
    if (!on) {                                                               /* whatever still reads the buffers has to be done before they go */
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        loudness_release(ctx);
    }
    ctx->loud.on = on;
    return GDG_OK;
}

static int own_buffer(gdg_ctx *ctx, double **d, size_t *cap, size_t bytes, bool *fresh) {
    *fresh = false;
    if (bytes <= *cap) return GDG_OK;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    drop(d, cap);
    if (hipMalloc((void **)d, bytes) != hipSuccess) return fail(ctx, GDG_ERR_NOMEM, "the loudness records cannot allocate %zu bytes on the device", bytes);
    *cap = bytes;
    *fresh = true;
    return GDG_OK;
}

int loudness_slice_begin(gdg_ctx *ctx, int ports, size_t pos, size_t samples, uint32_t rate) {
    gdg_ctx::Loudness &L = ctx->loud;
    L.valid = L.live = false;
    if (!L.on) return GDG_OK;
    if (!gdg_loudness_rate_ok(rate))
        return fail(ctx, GDG_ERR_INVALID, "the loudness records are on (gdg_batch_loudness_enable) and the session rate is %u; a hop is a tenth of a second in whole samples: a multiple of 10 from 8000 on", rate);
    const size_t hops = (size_t)gdg_loudness_hops_in(rate, pos, samples);
    bool fresh = false, fresh_records = false;
    int r;
    if ((r = own_buffer(ctx, &L.d_state, &L.state_cap, (size_t)ports * LOUDNESS_STATE * sizeof(double), &fresh)) != GDG_OK) return r;
    if (fresh && pos != 0) return fail(ctx, GDG_ERR_INVALID, "the loudness state of the open job has gone (gdg_batch_loudness_enable or gdg_batch_release between two slices?)");
    if ((r = own_buffer(ctx, &L.d_records, &L.records_cap, ((size_t)ports * hops + 1) * sizeof(double), &fresh_records)) != GDG_OK) return r;
    if (pos == 0) HIP_TRY(ctx, hipMemsetAsync(L.d_state, 0, (size_t)ports * LOUDNESS_STATE * sizeof(double), ctx->stream));
    L.ports = ports;
    L.hops = hops;
    L.hop_base = pos / gdg_loudness_hop(rate);
    L.rate = rate;
    L.par = gdg_loudness_params_at(rate);
    L.live = true;
    return GDG_OK;
}

int loudness_step(gdg_ctx *ctx, const double *d_rows, size_t row_stride, size_t first, size_t count) {
    gdg_ctx::Loudness &L = ctx->loud;
    if (!L.live) return GDG_OK;
    HIP_TRY(ctx, gdg_launch_block_loudness(d_rows, row_stride, (unsigned)L.ports, first, count, L.rate, L.hop_base, L.hops, L.par, L.d_state, L.d_records, ctx->stream));
    return GDG_OK;
}

int loudness_slice_end(gdg_ctx *ctx, int rc) {
    gdg_ctx::Loudness &L = ctx->loud;
    L.valid = L.live && rc == GDG_OK;
    L.live = false;
    return rc;
}

/* capacity in doubles */
int gdg_batch_loudness(gdg_ctx *ctx, double *records, size_t capacity, int *ports, size_t *hops) {
    if (!ctx) return GDG_ERR_INVALID;
    const gdg_ctx::Loudness &L = ctx->loud;
    if (!L.valid)
        return fail(ctx, GDG_ERR_INVALID, "no loudness records: the last batch call of this context %s",
                    L.on ? "has not completed, was a master finish, or none has run since gdg_batch_loudness_enable" : "ran without them (gdg_batch_loudness_enable comes before the call)");
    if (ports) *ports = L.ports;
    if (hops) *hops = L.hops;
    if (!records) return GDG_OK;
    const size_t n = (size_t)L.ports * L.hops;
    if (capacity < n) return fail(ctx, GDG_ERR_INVALID, "batch loudness: room for %zu doubles, the call has %d ports x %zu hops = %zu", capacity, L.ports, L.hops, n);
    if (!n) return GDG_OK;
    enter(ctx, /*read_only=*/true);
    HIP_TRY(ctx, hipMemcpyAsync(records, L.d_records, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GDG_OK;
}
