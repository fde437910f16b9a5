/*
 * api_batch.cpp -- controller.processFiles on the device: gdg_batch_run, its sharded form, the streamed form of both (slices of whole
 * blocks) and the master mix of a job and of a slice.
 * Part of the host side of libgdg.so (the C-ABI of include/gdg.h on top of the HIP kernels; see ctx.h for the map).
 * There is no CPU compute path here: every sample is produced by a HIP kernel.
 */
#include "ctx.h"
#include "batch_steps.h"
#include <future>

#define GDG_BLOCK_SIZE 8192           /* controller/controller.go:36 */

/* resample/resample.go:72-87 with 64-bit lengths (gdg_resample_time_length for files of any length; a rate of 0: nothing) */
static size_t resample_length64(size_t n, uint32_t source_rate, uint32_t target_rate) {
    if (source_rate == 0 || target_rate == 0) return 0;
    const double expansion = (double)target_rate / (double)source_rate;
    const double out_len_f = (double)n * expansion, out_len_floor = floor(out_len_f);
    long long out_len = (long long)out_len_floor;
    if (out_len_floor == out_len_f) out_len--;
    return out_len < 0 ? 0 : (size_t)out_len;
}

/* the samples an input covers in a job at target_rate: its (resampled) length, controller.go:2993-2999; none without bytes */
static size_t input_covers(const gdg_batch_input &in, uint32_t target_rate) {
    if (!in.bytes || !in.samples_per_channel) return 0;
    return in.sample_rate == target_rate ? in.samples_per_channel : resample_length64(in.samples_per_channel, in.sample_rate, target_rate);
}

/* every channel is padded to the longest input, in whole blocks (controller.go:3005-3016) */
static size_t whole_blocks(size_t samples) {
    return samples % GDG_BLOCK_SIZE ? GDG_BLOCK_SIZE * (samples / GDG_BLOCK_SIZE + 1) : samples;
}

int gdg_batch_length(gdg_ctx *ctx, const gdg_batch_input *inputs, int n_inputs, uint32_t target_rate, size_t *samples) {
    if (!ctx || !inputs || !samples || n_inputs <= 0) return GDG_ERR_INVALID;
    size_t max_len = 0;
    for (int i = 0; i < n_inputs; i++) {
        if (inputs[i].bytes && inputs[i].samples_per_channel > 0x7fffffff) return fail(ctx, GDG_ERR_INVALID, "input %d is too long", i);
        max_len = std::max(max_len, input_covers(inputs[i], target_rate));
    }
    *samples = whole_blocks(max_len);
    return GDG_OK;
}

/* slot i of the batch run's device buffers (ctx.h: BATCH_INPUTS ..) with at least `bytes` */
static int batch_buffer(gdg_ctx *ctx, int i, size_t bytes, void **out) {
    if (bytes > ctx->batch_dev_cap[i]) {
        hipFree(ctx->batch_dev[i]);
        ctx->batch_dev[i] = nullptr;
        ctx->batch_dev_cap[i] = 0;
        if (hipMalloc(&ctx->batch_dev[i], bytes) != hipSuccess) return fail(ctx, GDG_ERR_NOMEM, "the batch run cannot allocate %zu bytes on the device", bytes);
        ctx->batch_dev_cap[i] = bytes;
    }
    *out = ctx->batch_dev[i];
    return GDG_OK;
}

/* the slots `slots` go: freed, and made anew at the size then asked for by the next batch_buffer.  Whatever still reads them is done (the caller has waited). */
static void batch_drop(gdg_ctx *ctx, std::initializer_list<int> slots) {
    for (int i : slots) {
        hipFree(ctx->batch_dev[i]);
        ctx->batch_dev[i] = nullptr;
        ctx->batch_dev_cap[i] = 0;
    }
}

/* A history the job carries from slice to slice in slot `slot`, `bytes` long: the job's first slice (pos == 0) begins from zeros, every later one
 * from what the slice before left -- which is lost when the slot had to be made (gdg_batch_release between two slices).  `whose` words that. */
static int carried_history(gdg_ctx *ctx, int slot, size_t bytes, size_t pos, const char *whose, double **d) {
    const bool fresh = ctx->batch_dev_cap[slot] < bytes;
    if (const int r = batch_buffer(ctx, slot, bytes, (void **)d)) return r;
    if (fresh && pos != 0) return fail(ctx, GDG_ERR_INVALID, "the %s history of the open job is gone (gdg_batch_release between two slices?)", whose);
    if (pos == 0) HIP_TRY(ctx, hipMemsetAsync(*d, 0, bytes, ctx->stream));
    return GDG_OK;
}

/* the frames every resampled input keeps for its next step: the same few bytes for every job of the context's channels */
int batch_carry_buffer(gdg_ctx *ctx, double **d_carry) {
    return batch_buffer(ctx, BATCH_CARRY, (size_t)ctx->nch * GDG_STREAM_CARRY * sizeof(double), (void **)d_carry);
}

int gdg_batch_release(gdg_ctx *ctx) {
    if (!ctx) return GDG_ERR_INVALID;
    if (ctx->bstream.open) return fail(ctx, GDG_ERR_INVALID, "a streamed batch run is open on this context: its buffers are in use");
    enter(ctx);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < BATCH_DEV_SLOTS; i++) batch_drop(ctx, { i });
    loudness_release(ctx);
    return GDG_OK;
}

static int ensure_batch_pipe(gdg_ctx *ctx, size_t half_bytes, size_t up_half_bytes) {
    if (!ctx->batch_stream) {
        HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->batch_stream, hipStreamNonBlocking));
        HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->batch_up_stream, hipStreamNonBlocking));
        HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->batch_begin, hipEventDisableTiming));
        for (int h = 0; h < 2; h++) {
            HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->batch_ready[h], hipEventDisableTiming));
            HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->batch_moved[h], hipEventDisableTiming));
            HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->batch_up_ready[h], hipEventDisableTiming));
            for (int c = 0; c < 4; c++) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->batch_chunk[h][c], hipEventDisableTiming));
        }
    }
    HIP_TRY(ctx, ctx->h_up.grow(ctx, up_half_bytes));
    HIP_TRY(ctx, ctx->h_batch.grow(ctx, half_bytes));
    return GDG_OK;
}

/* host memcpy pieces (dst, src, bytes), spread over the copy threads */
struct BatchPiece { unsigned char *dst; const unsigned char *src; size_t bytes; };
static void move_pieces(gdg_ctx *ctx, const std::vector<BatchPiece> &pieces, int which = 0) {
    size_t total = 0;
    for (auto &p : pieces) total += p.bytes;
    copy_rows_parallel(ctx, 0, pieces.size(), [&](size_t i) { memcpy(pieces[i].dst, pieces[i].src, pieces[i].bytes); },
                       pieces.empty() ? 0 : total / pieces.size(), which);
}

/* ---- the block loop of one slice of a batch job -------------------------------------------------------------------------------------- */
struct BatchLoop {
    int N, enc_rows, f64_rows, out_width, W;
    size_t length;                              /* samples of every row of d_inputs = the samples this loop walks */
    size_t ws, enc_bytes;
    double *d_inputs, *d_win;
    unsigned char *d_enc;
    const gdg_batch_options *opt;
    void *const *out_bytes;
    const gdg_batch_shard_out *shard;
    bool run_metro, has_input;                  /* has_input: some input has samples, which come with their step (stage) */
    int trace;
    double t_begin;
    size_t job_blocks, origin_blocks;           /* the slice of a job of job_blocks blocks that starts at block origin_blocks */
    ReportLive live;                            /* the render report's kinds this call collects: their sections ride behind each step's bytes (report_sections.h) */
    bool dither;                                /* the dithered encoders (gdg_batch_set_dither in force and an LPCM out_format) ... */
    uint64_t dither_first;                      /* ... and the job's sample index of this loop's first sample */
    const gdg_spectrum_bands *bands;            /* the band spectrum's launch argument; null = off */
    const std::vector<gdg_align_pairs> *align;  /* the alignment report: the measured ports of this call, a launch's worth to a piece; null = off */
    const double *d_trim;                       /* the output trim: the gains of the window's N + 3 rows on the device; null = off */
    /* the blend outputs: n_blends rows behind the window's N + 3 (0 = off, and always for a shard); their table on the device (blend.h) and
     * their output gains -- null = every one 1.0: the blend rows go through the plain or the dithered encoder */
    int n_blends;
    gdg_blend_view blend;
    const double *d_blend_gain;
    /* while a term reaches back (a delay, or taps behind the first): the context's history of the N chain rows -- what the step before left
     * of them, zeros at the job's start; null otherwise, and then no sample a term reads lies in front of the job */
    double *d_blend_history;
    /* the list records (report_sections.h: the blend fits, the Gram list, the tap fits, the transfer list, the delivered rows' records): per
     * kind the list's table on the host and on the device (null for the delivered rows' records, which have none), the entries it counts
     * and what it sends down per block; count 0 and a shape that is off = off, and always for a shard */
    struct List { const int *h_table, *d_table; int count; ListShape shape; } list[LIST_KINDS];
    /* the delivery (include/gdg.h, DELIVERY; deliver.h): the factor (0 or 1 = off, and always for a shard), the scratch rows [NR][ws / R] the
     * encoders read instead of the window, the factor's taps on the device and the window rows' history [NR][154] */
    int deliver;
    double *d_delivered, *d_deliver_history;
    const double *d_deliver_taps;
    /* ... and the ratio behind it (0 / 0 or 1 / 1 = off, and always for a shard): the rows behind the ratio stage, [NR][ratio_stride], which the
     * encoders then read, the ratio's [T][up] table on the device and the intermediate rows' history [NR][127] */
    int ratio_up, ratio_down;
    double *d_ratio_rows, *d_ratio_history;
    const double *d_ratio_taps;
    size_t ratio_stride;
    /* what the records of the delivered rows (list[LIST_DELIVERED]; include/gdg.h, DELIVERED RECORDS) read beside the rows: the 23 samples every
     * encoded row keeps from step to step, [NR][23], and room for the steps' block spans on the device */
    double *d_out_rec_history;
    unsigned long long *d_out_rec_spans;
};

/* the inputs of step i (samples [off, off + w * 8192) of the loop) go up: gathered into a pinned half, moved and decoded on the upload stream */
typedef std::function<int(size_t i, size_t off, int w, int pool)> BatchStage;

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

/* ---- the three record kinds that are taken port by port: block statistics, band spectrum, true peak ----------------------------------- */
/* rows that are measured as they lie: n_rows rows `stride` samples apart, whose records begin at record row first_rec of a kind's section */
struct RowGroup { const double *rows; size_t stride; unsigned n_rows; size_t first_rec; };
/* what the band spectrum's launch reads beside the rows */
struct SpectrumTables { const gdg_spectrum_bands *bands; const double *win; double2 *tw, *tw2; };

/* The launches of `kinds` (of REPORT_STATS, REPORT_BANDS and REPORT_TRUE_PEAK; one that is not live is passed over) over `samples` samples of
 * every group's rows, the kinds in the outer loop: a group's records of kind k go to the rows [first_rec ..] of k's section [rows][w] in `enc` */
static int port_records(gdg_ctx *ctx, std::initializer_list<int> kinds, const RowGroup *groups, int n_groups, size_t samples, size_t w, const ReportLive &live,
                        const ReportSections &sec, unsigned char *enc, const SpectrumTables &spec) {
    for (int k : kinds) {
        if (!live.on(k)) continue;
        for (int g = 0; g < n_groups; g++) {
            const RowGroup &G = groups[g];
            unsigned char *rec = enc + sec.at[k] + G.first_rec * w * live.elem[k];
            if (k == REPORT_STATS) HIP_TRY(ctx, gdg_launch_block_stats(G.rows, G.stride, G.n_rows, samples, (unsigned)GDG_BLOCK_SIZE, rec, ctx->stream));
            else if (k == REPORT_BANDS)
                HIP_TRY(ctx, gdg_launch_block_spectrum(G.rows, G.stride, G.n_rows, samples, spec.win, spec.tw, spec.tw2, *spec.bands, reinterpret_cast<double *>(rec), ctx->stream));
            else HIP_TRY(ctx, gdg_launch_block_true_peak(G.rows, G.stride, G.n_rows, samples, true_peak_table(), rec, ctx->stream));
        }
    }
    return GDG_OK;
}

namespace {                                     /* nothing of the loop leaves this file */
/* a step of the loop: the blocks [off / 8192, off / 8192 + w) of the slice (batch_steps.h), the sections behind its rows (report_sections.h) and
 * where its block spans begin among the slice's (the delivered rows' records) */
struct Step { size_t off; int w; ReportSections sec; ListSections lists; size_t span_at; };

/* The block loop, controller.go:3076-3107 around controller.process (:2648-2783), `w` blocks per step: the steps of the slice `p` and what each
 * of them enqueues on the compute, the download and (through stage_fn) the upload stream.  plan() lays the steps out, run() drives them. */
struct BlockLoop {
    static constexpr int B = GDG_BLOCK_SIZE;
    gdg_ctx *const ctx;
    const BatchLoop &p;
    const BatchStage &stage_fn;
    const int NO, NR;                           /* the window's N + 3 rows, and with the blends' behind them */
    const int R, RL, RM;                        /* the delivery factor: every byte count below is of the delivered length (deliver.h); the ratio behind it; 1 / 1: none */
    const bool ratio, sharded;
    const size_t rec_rows;                      /* the record rows of a section: N + 3 and the blends', a shard's N chain rows and the metronome's */
    std::vector<Step> steps;
    /* the rows of a section that are filed: every row (a shard without the metronome: that row stays zero); of the alignment records only
     * the measured ports' are written, and read */
    std::vector<size_t> filed[REPORT_KINDS];
    SpectrumTables spec = { nullptr, nullptr, nullptr, nullptr };
    double2 *align_tw = nullptr, *transfer_tw = nullptr;
    std::future<int> staged;                    /* the helper thread's gather in flight */
    const std::vector<int> *helper_cpus = nullptr;

    BlockLoop(gdg_ctx *ctx, const BatchLoop &p, const BatchStage &stage_fn)
        : ctx(ctx), p(p), stage_fn(stage_fn), NO(p.N + 3), NR(p.N + 3 + p.n_blends), R(p.deliver > 1 ? p.deliver : 1), RL(p.ratio_up > 0 ? p.ratio_up : 1),
          RM(p.ratio_down > 0 ? p.ratio_down : 1), ratio(gdg_deliver_ratio_on(RL, RM)), sharded(p.shard != nullptr), rec_rows(sharded ? (size_t)p.N + 1 : (size_t)NR) {}
    ~BlockLoop() { if (staged.valid()) staged.wait(); }                      /* the helper thread works on this object */

    /* a step's delivered rows: the loop begins at session sample p.dither_first of its job, and a ratio counts in job indices */
    DeliverStep step_of(size_t w, size_t off, size_t rows) const { return deliver_ratio_step(w, off, (size_t)p.dither_first, R, RL, RM, (size_t)p.out_width, rows); }
    int pieces(size_t i) const { return step_pieces(steps[i].w, p.enc_rows); }
    size_t piece_row(size_t i, int c) const { return deliver_chunk_row((size_t)p.enc_rows, c, pieces(i)); }      /* first encoded row of piece c */
    double *master() const { return p.d_win + (size_t)p.N * p.ws; }
    double *metro() const { return master() + 2 * p.ws; }
    unsigned char *enc_half(size_t i) const { return p.d_enc + (i & 1) * p.enc_bytes; }

    /* what step i sends down: its encoded rows (and a shard's float64 rows), compact; behind them one section per live kind of the render
     * report, [rows][w] -- N + 3 rows and the blends', a shard's N chain rows and the metronome's -- which come down with the last piece */
    size_t down_bytes(size_t i) const {
        const size_t wb = (size_t)steps[i].w * B, row_bytes = step_of((size_t)steps[i].w, steps[i].off, 0).row_bytes;
        return sharded ? (((size_t)p.enc_rows * row_bytes + 15) & ~(size_t)15) + (size_t)p.f64_rows * wb * sizeof(double) : (size_t)NR * row_bytes;
    }

    /* the steps (batch_steps.h), every step's sections, the delivered rows' spans, the filed rows and the kinds' tables */
    int plan() {
        int r;
        if (ctx->all_channels.empty()) for (int c = 0; c < ctx->nch; c++) ctx->all_channels.push_back(c);
        for (const SliceStep &s : slice_steps(p.job_blocks, p.origin_blocks, p.length / B, p.W)) steps.push_back({ s.off * B, s.w, {}, {}, 0 });
        ListShape list_shape[LIST_KINDS];
        for (int k = 0; k < LIST_KINDS; k++) list_shape[k] = p.list[k].shape;
        for (size_t i = 0; i < steps.size(); i++) {
            steps[i].sec = report_sections(p.live, rec_rows, (size_t)steps[i].w, down_bytes(i), true);
            steps[i].lists = list_sections(steps[i].sec.end, list_shape, (size_t)steps[i].w);        /* behind the last of them: [fits][w], [w], [w], [w], [NR][w] */
        }
        /* the delivered rows' blocks: session block j of a step delivers the samples [span[j], span[j + 1]) of the step's rows, counted where every
         * other count of a delivered step comes from (deliver.h); all steps' spans go up once, ahead of everything the loop enqueues */
        if (p.list[LIST_DELIVERED].count) {
            std::vector<unsigned long long> &spans = ctx->out_rec_spans;
            spans.clear();
            for (Step &st : steps) {
                st.span_at = spans.size();
                for (int j = 0; j <= st.w; j++) spans.push_back((unsigned long long)step_of((size_t)j, st.off, 0).samples);
            }
            HIP_TRY(ctx, hipMemcpyAsync(p.d_out_rec_spans, spans.data(), spans.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, ctx->stream));
        }
        for (int k = 0; k < REPORT_KINDS; k++) {
            if (!p.live.on(k)) continue;
            if (k == REPORT_ALIGN) { for (const gdg_align_pairs &q : *p.align) for (int j = 0; j < q.n; j++) filed[k].push_back((size_t)q.port[j]); }
            else for (size_t o = 0; o < ((sharded && !p.run_metro) ? (size_t)p.N : rec_rows); o++) filed[k].push_back(o);
        }
        spec.bands = p.bands;
        if (p.bands && (r = spectrum_tables(ctx, &spec.win, &spec.tw, &spec.tw2)) != GDG_OK) return r;
        double2 *align_tw2 = nullptr;
        if (p.align && (r = fir_tables(ctx, GDG_ALIGN_BLOCK, &align_tw, &align_tw2)) != GDG_OK) return r;
        if (p.list[LIST_TRANSFER].count && (r = fir_tables(ctx, GDG_TRANSFER_BLOCK, &transfer_tw, &align_tw2)) != GDG_OK) return r;      /* the same transform's tables as the alignment's */
        return GDG_OK;
    }

    /* step i's bytes from its pinned half into the files */
    int scatter(size_t i) {
        const Step &st = steps[i];
        const unsigned char *src = ctx->h_batch[i & 1];
        const DeliverStep ds = step_of((size_t)st.w, st.off, (size_t)p.enc_rows);
        const size_t wb = (size_t)st.w * B, row_bytes = ds.row_bytes, at = ds.file_at, enc_rows = (size_t)p.enc_rows;
        const size_t f64_at = (enc_rows * row_bytes + 15) & ~(size_t)15;
        const int K = pieces(i);
        for (int c = 0; c < K; c++) {
            HIP_TRY(ctx, hipEventSynchronize(ctx->batch_chunk[i & 1][c]));    /* piece c has landed */
            const size_t o0 = piece_row(i, c), o1 = (c + 1 == K) ? enc_rows + (size_t)p.f64_rows : piece_row(i, c + 1);
            copy_rows_parallel(ctx, o0, o1, [&](size_t o) {
                if (o < enc_rows) {
                    /* NULL: "skipping output" (:3143); a shard's row N is the metronome track */
                    void *dst = (sharded && o == (size_t)p.N) ? p.shard->metronome_bytes : p.out_bytes[o];
                    if (dst) memcpy(static_cast<unsigned char *>(dst) + at, src + o * row_bytes, ds.copy_bytes);      /* without a ratio the whole row; with one its samples, not the pad */
                } else {
                    const size_t k = o - enc_rows;
                    double *dst = k == 0 ? p.shard->master_left : (k == 1 ? p.shard->master_right : p.shard->metronome);
                    memcpy(dst + st.off, src + f64_at + k * wb * sizeof(double), wb * sizeof(double));
                }
            }, row_bytes);
        }
        for (int k = 0; k < REPORT_KINDS; k++)                               /* the last piece brought the step's sections: filed under the step's blocks */
            if (p.live.on(k)) report_file(ctx, k, src + st.sec.at[k], filed[k], (size_t)st.w, st.off / B);
        for (int k = 0; k < LIST_KINDS; k++)
            if (p.list[k].count) list_file(ctx, k, src + st.lists.of[k].at, (size_t)st.w, st.off / B);
        return GDG_OK;
    }

    int stage(size_t i, int pool = 0) {
        if (!p.has_input || i >= steps.size()) return GDG_OK;
        return stage_fn(i, steps[i].off, steps[i].w, pool);
    }

    /* step i's chain: the block loop's work for its w blocks, which fill the first w * 8192 samples of the window's rows */
    int chain(size_t i) {
        const int N = p.N, w = steps[i].w, wb = w * B;
        const size_t ws = p.ws, length = p.length;
        const uint32_t rate = p.opt->target_rate;
        const double *d_in = p.d_inputs + steps[i].off;
        double *d_master = master(), *d_metro = metro();
        int r;
        if (p.opt->tuner_enqueue)
            for (int j = 0; j < w; j++) if ((r = tuner_enqueue_rows(ctx, d_in + (size_t)j * B, length, B, rate)) != GDG_OK) return r;
        if ((r = process_rows(ctx, ctx->all_channels, d_in, p.d_win, B, rate, (int)length, false, 1, nullptr, nullptr, w, (int)ws)) != GDG_OK) return r;
        if (p.run_metro && (r = gdg_metronome_process_device(ctx, d_metro, wb)) != GDG_OK) return r;
        /* the step's w frames are consecutive in their rows: ONE mix over w x 8192 samples gives the samples of w calls (a frame's first
         * samples find their delayed neighbours in the frame before instead of in the history, which holds the same values) */
        if ((r = spatialize_rows(ctx, p.d_win, (int)ws, d_master, (int)ws, wb)) != GDG_OK) return r;
        /* a shard's master rows stay partial sums: the aux input is added once, after the shards' sums (gdg_batch_finish_master) */
        if (p.opt->metronome_to_master && !sharded) HIP_TRY(ctx, gdg_launch_add_aux(d_master, d_master + ws, d_metro, wb, ctx->stream));
        if (p.opt->run_meters) {                                             /* ports: inputs | outputs | metronome | left, right (:2707-2777) */
            if ((r = meter_rows(ctx, d_in, length, 0, N, wb, rate)) != GDG_OK) return r;
            if ((r = meter_rows(ctx, p.d_win, ws, N, N, wb, rate)) != GDG_OK) return r;
            if (p.run_metro && (r = meter_rows(ctx, d_metro, ws, 2 * N, 1, wb, rate)) != GDG_OK) return r;
            if (!sharded && (r = meter_rows(ctx, d_master, ws, 2 * N + 1, 2, wb, rate)) != GDG_OK) return r;     /* a shard's master ports: gdg_batch_finish_master */
        }
        return GDG_OK;
    }

    /* ... the blend rows and the records of the window's rows as the encoder is about to read them, into the sections of the step's half of `enc` */
    int records(size_t i) {
        const Step &st = steps[i];
        const int N = p.N, w = st.w;
        const size_t ws = p.ws, wb = (size_t)w * B;
        unsigned char *enc = enc_half(i);
        /* the blend rows, behind the metronome's: sums of the chain rows, which are final; every reader below takes them as rows like the others */
        if (p.n_blends) {
            /* terms that reach back read the step before: its tail is the history (a step has at least 8192 samples, a term reaches at most
             * 4096 back).  This step's tail replaces it behind the sum and before the next step writes the window. */
            HIP_TRY(ctx, gdg_launch_blend(p.blend, p.d_win, ws, wb, p.d_blend_history, (size_t)GDG_BLEND_MAX_DELAY, p.d_win + (size_t)NO * ws, ws, ctx->stream));
            if (p.d_blend_history) HIP_TRY(ctx, gdg_launch_blend_history_save(p.d_win, ws, wb, (unsigned)N, p.d_blend_history, ctx->stream));
        }
        /* the loudness records (api_loudness.cpp; off: nothing): the same rows, the job's samples from this step's first on */
        if (const int rl = loudness_step(ctx, p.d_win, ws, (size_t)p.dither_first + st.off, wb)) return rl;
        /* statistics, then the band spectrum: the window's rows, and a shard's metronome row, which is row N + 2 of the window and record row N */
        const unsigned n_win = sharded ? (unsigned)N : (unsigned)NR;
        const RowGroup groups[2] = { { p.d_win, ws, n_win, 0 }, { metro(), ws, 1u, (size_t)N } };
        const int n_groups = (sharded && p.run_metro) ? 2 : 1;
        int r;
        if ((r = port_records(ctx, { REPORT_STATS, REPORT_BANDS }, groups, n_groups, wb, (size_t)w, p.live, st.sec, enc, spec)) != GDG_OK) return r;
        if (p.align)                                                         /* ... the same rows, one more reader: a shard's metronome port is row N + 2, as metro() is */
            for (const gdg_align_pairs &q : *p.align)
                HIP_TRY(ctx, gdg_launch_block_align(p.d_win, ws, n_win, (unsigned)N + 2u, (unsigned)rec_rows, wb, q, align_tw, enc + st.sec.at[REPORT_ALIGN], ctx->stream));
        /* ... and the inter-sample peaks of the same rows */
        if ((r = port_records(ctx, { REPORT_TRUE_PEAK }, groups, n_groups, wb, (size_t)w, p.live, st.sec, enc, spec)) != GDG_OK) return r;
        /* the list records of the same rows, the blends' among them: the fits' inner products, then the Gram of the listed rows and the
         * tap fits' Gram of shifted rows on the matrix cores */
        for (int k = 0; k < LIST_LAUNCHERS; k++)
            if (p.list[k].count)
                HIP_TRY(ctx, list_launch[k](p.d_win, ws, (unsigned)NR, wb, (unsigned)B, p.list[k].h_table, p.list[k].d_table, (unsigned)p.list[k].count, enc + st.lists.of[k].at, ctx->stream));
        /* ... and the transfer records of the same rows: a block of the loop is a block of the record (8192 samples) */
        if (const BatchLoop::List &T = p.list[LIST_TRANSFER]; T.count)
            HIP_TRY(ctx, gdg_launch_block_transfer(p.d_win, ws, (unsigned)NR, wb, T.h_table, T.d_table, (unsigned)T.count, transfer_tw, enc + st.lists.of[LIST_TRANSFER].at, ctx->stream));
        return GDG_OK;
    }

    /* ... and the rows' way into the step's half of `enc`: the delivery, the ratio behind it, the records of the delivered rows, the encoders */
    int deliver_encode(size_t i) {
        const Step &st = steps[i];
        const int N = p.N, w = st.w;
        const size_t ws = p.ws, wb = (size_t)w * B;
        unsigned char *enc = enc_half(i);
        const DeliverStep ds = step_of((size_t)w, st.off, 0);
        const size_t row_bytes = ds.row_bytes;
        /* dither on: n_chain rows are chain outputs from port_base on, the rows behind them the job-wide ones */
        /* trim on: `gains` = the gain of the launch's first row (the trim's in the window's order, the blends' own), null: none */
        /* delivered: the rows are the scratch rows' -- a row enc_stride apart (ws / R, behind a ratio its fixed pitch), ds.pitch samples of it (wb / R,
         * behind a ratio the step's count rounded up to four) -- and a sample's index is its index in the delivered job */
        const size_t enc_stride = ratio ? p.ratio_stride : ws / (size_t)R;
        auto encode_rows = [&](const double *rows, unsigned n_rows, unsigned n_chain, uint32_t port_base, unsigned char *dst, const double *gains) -> hipError_t {
            const gdg_encode_mode m = { gains != nullptr, p.dither, gains, { 1.0, 1.0 }, { ctx->dither_seed, (uint64_t)ds.first_out, port_base, n_chain } };
            return gdg_launch_wave_encode_rows(p.opt->out_format, rows, enc_stride, ds.pitch, n_rows, dst, m, ctx->stream);
        };
        /* the delivery: the window's NR rows, final by now and read by every record above as they are, decimated into the scratch rows -- the
         * samples in front of the step come from the history, which this step's tail replaces behind the launch and before the next step
         * writes the window.  The order is decimate, then gain, then the plain or dithered encoder: the encoders read the scratch rows. */
        const double *enc_src = p.d_win;
        if (R > 1) {
            HIP_TRY(ctx, gdg_launch_deliver_rows(R, p.d_win, ws, wb, (unsigned)NR, p.d_deliver_taps, p.d_deliver_history, p.d_delivered, ws / (size_t)R, ctx->stream));
            HIP_TRY(ctx, gdg_launch_deliver_history_save(p.d_win, ws, wb, (unsigned)NR, p.d_deliver_history, ctx->stream));
            enc_src = p.d_delivered;
        }
        /* ... and the ratio behind the factor: the intermediate rows (the window's at factor 1, the scratch rows otherwise) resampled into rows
         * of their own, +0.0 up to the pitch; their tail becomes the history before the next step writes them */
        if (ratio) {
            HIP_TRY(ctx, gdg_launch_deliver_ratio(RL, RM, enc_src, ws / (size_t)R, ds.inter_samples, (unsigned long long)ds.inter_first, (unsigned)NR, p.d_ratio_taps,
                                                  p.d_ratio_history, p.d_ratio_rows, p.ratio_stride, ds.pitch, ctx->stream));
            HIP_TRY(ctx, gdg_launch_deliver_ratio_history_save(enc_src, ws / (size_t)R, ds.inter_samples, (unsigned)NR, p.d_ratio_history, ctx->stream));
            enc_src = p.d_ratio_rows;
        }
        /* the records of the rows the encoders are about to read, in front of any gain: the step's w blocks as the delivery cut them, the 23
         * samples in front of the step from the history, which the step's tail replaces behind the launch */
        if (p.list[LIST_DELIVERED].count) {
            HIP_TRY(ctx, gdg_launch_block_delivered(enc_src, enc_stride, (unsigned)NR, ds.samples, p.d_out_rec_spans + st.span_at, (unsigned)w, p.d_out_rec_history,
                                                    true_peak_table(), enc + st.lists.of[LIST_DELIVERED].at, ctx->stream));
            HIP_TRY(ctx, gdg_launch_delivered_history_save(enc_src, enc_stride, ds.samples, (unsigned)NR, p.d_out_rec_history, ctx->stream));
        }
        if (!sharded) {
            HIP_TRY(ctx, encode_rows(enc_src, (unsigned)NO, (unsigned)N, ctx->dither_port_base, enc, p.d_trim));
            /* a launch of their own: blend b is port port_base + N + 3 + b of the dither, and its gain is the blend's, not the trim's */
            if (p.n_blends)
                HIP_TRY(ctx, encode_rows(enc_src + (size_t)NO * enc_stride, (unsigned)p.n_blends, (unsigned)p.n_blends, ctx->dither_port_base + (uint32_t)NO,
                                         enc + (size_t)NO * row_bytes, p.d_blend_gain));
            return GDG_OK;
        }
        HIP_TRY(ctx, encode_rows(p.d_win, (unsigned)N, (unsigned)N, ctx->dither_port_base, enc, p.d_trim));
        if (p.shard->metronome_bytes)
            HIP_TRY(ctx, encode_rows(metro(), 1u, 1u, GDG_DITHER_PORT_METRONOME, enc + (size_t)N * row_bytes, p.d_trim ? p.d_trim + N + GDG_TRIM_METRONOME : nullptr));
        unsigned char *f64 = enc + (((size_t)p.enc_rows * row_bytes + 15) & ~(size_t)15);
        HIP_TRY(ctx, hipMemcpy2DAsync(f64, wb * sizeof(double), master(), ws * sizeof(double), wb * sizeof(double), 2, hipMemcpyDeviceToDevice, ctx->stream));
        if (p.shard->metronome) HIP_TRY(ctx, hipMemcpyAsync(f64 + 2 * wb * sizeof(double), metro(), wb * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        return GDG_OK;
    }

    /* step i on the compute stream: its chain, then -- once step i - 2 has left the step's half of `enc` -- its records and the encoders into that half */
    int enqueue_compute(size_t i) {
        const int h = (int)(i & 1);
        int r;
        if (p.has_input) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->batch_up_ready[h], 0));
        if ((r = chain(i)) != GDG_OK) return r;
        if (i >= 2) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->batch_moved[h], 0));     /* step i - 2 has left enc */
        {
            ProfScope ps(ctx, GDG_K_WAVE);
            if ((r = records(i)) != GDG_OK || (r = deliver_encode(i)) != GDG_OK) return r;
        }
        HIP_TRY(ctx, hipEventRecord(ctx->batch_ready[h], ctx->stream));
        return GDG_OK;
    }

    /* ... and its way down on the download stream, into the step's pinned half (which step i - 2 must have left: scatter(i - 2) is done), in
     * pieces(i) pieces of whole rows (batch_steps.h; the float64 rows of a shard and the sections ride with the last one), an event behind each */
    int enqueue_down(size_t i) {
        const int h = (int)(i & 1);
        unsigned char *enc = enc_half(i);
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->batch_stream, ctx->batch_ready[h], 0));
        const size_t row_bytes = step_of((size_t)steps[i].w, steps[i].off, 0).row_bytes;
        const size_t down = steps[i].lists.end;
        const int K = pieces(i);
        for (int c = 0; c < K; c++) {
            size_t b0 = 0, b1 = 0;
            deliver_chunk_bytes((size_t)p.enc_rows, row_bytes, c, K, down, &b0, &b1);
            if (b1 > b0) HIP_TRY(ctx, hipMemcpyAsync(ctx->h_batch[h] + b0, enc + b0, b1 - b0, hipMemcpyDeviceToHost, ctx->batch_stream));
            HIP_TRY(ctx, hipEventRecord(ctx->batch_chunk[h][c], ctx->batch_stream));
        }
        HIP_TRY(ctx, hipEventRecord(ctx->batch_moved[h], ctx->batch_stream));
        return GDG_OK;
    }

    /* stage(first .. last), one after the other, on the helper thread */
    void on_helper(size_t first, size_t last) {
        if (first >= steps.size()) return;
        try {
            staged = std::async(std::launch::async, [this, first, last]() -> int {
                if (helper_cpus) numa_bind_thread(*helper_cpus);
                if (hipSetDevice(ctx->device) != hipSuccess) return GDG_ERR_HIP;
                for (size_t k = first; k <= last && k < steps.size(); k++) { const int rr = stage(k, 1); if (rr != GDG_OK) return rr; }
                return GDG_OK;
            });
        } catch (...) {                                                    /* no thread to be had: gather here, as the short runs do */
            int rr = GDG_OK;
            for (size_t k = first; k <= last && k < steps.size() && rr == GDG_OK; k++) rr = stage(k, 0);
            std::promise<int> done;
            done.set_value(rr);
            staged = done.get_future();
        }
    }

    int run() {
        int r;
        HIP_TRY(ctx, hipEventRecord(ctx->batch_begin, ctx->stream));         /* rows zeroed */
        if (p.has_input) HIP_TRY(ctx, hipStreamWaitEvent(ctx->batch_up_stream, ctx->batch_begin, 0));
        /* The compute stream is kept TWO steps ahead of the files.  Round 2 enqueued step i + 1 only after step i - 1 had been scattered into
         * the caller's buffers, which closed a loop of compute -> download -> scatter over two steps: (5.7 + 4.0 + 3.1) / 2 = 6.4 ms per step
         * of 16 blocks where the device needs 5.7 (GDG_BATCH_TRACE).  Now step i + 2 is enqueued as soon as step i's download has finished (before
         * its bytes are scattered), while step i + 1 is already queued behind step i on the device. */
        if (p.trace) fprintf(stderr, "[batch] set-up %.2f ms\n", now_ms() - p.t_begin);
        /* Gathering step i + 2's input bytes (1.9 ms of 16 blocks x 512 files) and scattering step i's output bytes (3.0 ms) were one thread's
         * work, one after the other: 4.8 ms per step beside the device's 4.7 -- the host set the pace half of the time.  With windows of four
         * blocks or more the gather runs on a helper thread with copy workers of its own (copy_pool_up), one step further ahead (step i + 3 while
         * step i is scattered; its pinned half and its device half were step i + 1's, whose upload and decode are long done -- stage() waits
         * for their event): the host's step is the scatter alone and the device sets the pace. */
        const bool helper = p.has_input && p.ws >= (size_t)4 * B && steps.size() > 3;
        /* the upload side's copy workers are made HERE, by the caller's thread, and the helper thread goes where they go: with option "numa" = 2
         * workers are bound to the node of the thread that makes them, and a helper the scheduler happened to start on the other socket would
         * put the gather's workers a socket away from the caller's buffers and the pinned halves */
        if (helper) { ensure_copy_pool(ctx, 1); numa_target(ctx, &helper_cpus); }
        if (helper) {
            /* the head: step 0 is gathered here; steps 1 and 2 on the helper meanwhile, so that the first whole window's bytes are on the bus
             * while the quarter and the half window compute */
            if ((r = stage(0)) != GDG_OK) return r;
            on_helper(1, 2);
            if ((r = enqueue_compute(0)) != GDG_OK || (r = enqueue_down(0)) != GDG_OK) return r;
            if ((r = staged.get()) != GDG_OK) return r;
            if ((r = enqueue_compute(1)) != GDG_OK || (r = enqueue_down(1)) != GDG_OK) return r;
        } else {
            for (size_t i = 0; i < 2 && i < steps.size(); i++) {
                if ((r = stage(i)) != GDG_OK) return r;
                if ((r = enqueue_compute(i)) != GDG_OK || (r = enqueue_down(i)) != GDG_OK) return r;
            }
        }
        if (p.trace) fprintf(stderr, "[batch] steps 0 and 1 staged and enqueued at %.2f ms\n", now_ms() - p.t_begin);
        for (size_t i = 0; i < steps.size(); i++) {
            const double t_it = now_ms();
            if (helper) {
                if (staged.valid() && (r = staged.get()) != GDG_OK) return r;     /* step i + 2's inputs are on their way up (i = 0: since the head) */
                on_helper(i + 3, i + 3);
            } else if ((r = stage(i + 2)) != GDG_OK) return r;                   /* while steps i, i + 1 run: the inputs of step i + 2 go up ... */
            const double t_st = now_ms();
            const double t_wait = t_st;
            /* step i + 2 needs step i's half of `enc` (the compute stream waits for its download itself) but not its pinned half: it goes onto
             * the compute stream BEFORE the scatter, so the loop compute -> download -> compute spans 5.7 + 4.0 ms per two steps and the device,
             * not the host, sets the pace */
            if (i + 2 < steps.size() && (r = enqueue_compute(i + 2)) != GDG_OK) return r;
            const double t_enq = now_ms();
            if ((r = scatter(i)) != GDG_OK) return r;                            /* ... step i comes down and goes into the files, piece by piece */
            if (i + 2 < steps.size() && (r = enqueue_down(i + 2)) != GDG_OK) return r;     /* its pinned half is free again */
            if (p.trace) fprintf(stderr, "[batch] step %zu (w %d): stage %zu %.2f | (%.2f) | enqueue %zu %.2f | download + scatter %.2f  (at %.2f ms)\n", i, steps[i].w, i + 2,
                                 t_st - t_it, t_wait - t_st, i + 2, t_enq - t_wait, now_ms() - t_enq, now_ms() - p.t_begin);
        }
        return check_device_error(ctx);
    }
};
}

static int batch_block_loop(gdg_ctx *ctx, const BatchLoop &p, const BatchStage &stage_fn) {
    BlockLoop loop(ctx, p, stage_fn);
    const int r = loop.plan();
    return r != GDG_OK ? r : loop.run();
}

/* ================================================================================================
 * A batch job runs in slices of whole blocks (the one-call run: in one).  Every input comes with its step -- decoded (with the channel
 * pick) straight into its row, or into the resampler's source buffer behind the frames kept from the step before -- so the device holds
 * one slice of decoded input and nothing of the files' length.
 * ============================================================================================== */
/* GDG_STREAM_CARRY (ctx.h): the source frames kept per resampled input */

int gdg_batch_stream_span(size_t samples_per_channel, uint32_t source_rate, uint32_t target_rate, size_t out_first, size_t out_count,
                          size_t *src_first, size_t *src_count) {
    if (!src_first || !src_count || source_rate == 0 || target_rate == 0) return GDG_ERR_INVALID;
    const size_t n = samples_per_channel;
    const size_t covered = source_rate == target_rate ? n : resample_length64(n, source_rate, target_rate);
    if (out_first >= covered || out_count == 0) { *src_first = n; *src_count = 0; return GDG_OK; }      /* zero padding: no source frame */
    const size_t out_end = out_count > covered - out_first ? covered : out_first + out_count;
    if (source_rate == target_rate) { *src_first = out_first; *src_count = out_end - out_first; return GDG_OK; }
    const double dx = (double)source_rate / (double)target_rate;                                     /* resample.go:88-90 */
    long long lo = (long long)floor((double)out_first * dx) - 2, hi = (long long)floor((double)(out_end - 1) * dx) + 4;
    if (lo < 0) lo = 0;
    if (hi > (long long)n) hi = (long long)n;
    if (hi < lo) hi = lo;
    *src_first = (size_t)lo;
    *src_count = (size_t)(hi - lo);
    return GDG_OK;
}

/* the source map: validated whole before it replaces the one in force (batch_sources.h); read when a job is described */
int gdg_batch_set_sources(gdg_ctx *ctx, const int *source, int n) {
    if (!ctx) return GDG_ERR_INVALID;
    if (ctx->bstream.open) return fail(ctx, GDG_ERR_INVALID, "set sources: a streamed batch run is open on this context; its map holds until gdg_batch_stream_close");
    if (!source || n == 0) { ctx->batch_source.clear(); return GDG_OK; }
    int bad = -1;
    switch (sources_check(source, n, ctx->nch, &bad)) {
    case SOURCES_OK: break;
    case SOURCES_WRONG_N: return fail(ctx, GDG_ERR_INVALID, "set sources: a map of %d entries, the context has %d channels", n, ctx->nch);
    case SOURCES_OUT_OF_RANGE: return fail(ctx, GDG_ERR_INVALID, "set sources: channel %d reads channel %d, the context has channels 0 to %d", bad, source[bad], ctx->nch - 1);
    default:
        return fail(ctx, GDG_ERR_INVALID, "set sources: channel %d reads channel %d, which itself reads channel %d: a reader's source must read its own input",
                    bad, source[bad], source[source[bad]]);
    }
    ctx->batch_source.assign(source, source + n);
    return GDG_OK;
}

/* the dither of the LPCM outputs: validated whole before it replaces the setting in force; read by every call that encodes */
int gdg_batch_set_dither(gdg_ctx *ctx, int mode, uint64_t seed, uint32_t port_base) {
    if (!ctx) return GDG_ERR_INVALID;
    if (ctx->bstream.open) return fail(ctx, GDG_ERR_INVALID, "set dither: a streamed batch run is open on this context; its setting holds until gdg_batch_stream_close");
    if (mode != 0 && mode != 1) return fail(ctx, GDG_ERR_INVALID, "set dither: mode %d; 0 is off, 1 is TPDF", mode);
    if (mode != 0 && !gdg_dither_ports_ok(port_base, ctx->nch))              /* off: port_base is not used and cannot be wrong */
        return fail(ctx, GDG_ERR_INVALID, "set dither: port_base %u + %d channels reaches the job-wide ports from 0x%x on", port_base, ctx->nch, GDG_DITHER_PORT_MASTER_LEFT);
    ctx->dither_mode = mode;
    ctx->dither_seed = seed;
    ctx->dither_port_base = port_base;
    ctx->dither_cursor = 0;
    return GDG_OK;
}

/* the output trim: validated whole before it replaces the setting in force; read by every call that encodes (trim.h) */
int gdg_batch_set_trim(gdg_ctx *ctx, const double *chain_gain, int n, double master_left, double master_right, double metronome) {
    if (!ctx) return GDG_ERR_INVALID;
    if (ctx->bstream.open) return fail(ctx, GDG_ERR_INVALID, "set trim: a streamed batch run is open on this context; its setting holds until gdg_batch_stream_close");
    if (!(chain_gain == nullptr && n == 0) && (chain_gain == nullptr || n != ctx->nch))
        return fail(ctx, GDG_ERR_INVALID, "set trim: %d chain gains, the context has %d channels (NULL and 0: every chain gain 1)", n, ctx->nch);
    const int bad = chain_gain ? gdg_trim_first_nonfinite(chain_gain, n) : -1;
    if (bad >= 0) return fail(ctx, GDG_ERR_INVALID, "set trim: chain_gain[%d] = %g is not finite", bad, chain_gain[bad]);
    const double wide[3] = { master_left, master_right, metronome };
    static const char *const names[3] = { "master_left", "master_right", "metronome" };
    const int bad_wide = gdg_trim_first_nonfinite(wide, 3);
    if (bad_wide >= 0) return fail(ctx, GDG_ERR_INVALID, "set trim: %s = %g is not finite", names[bad_wide], wide[bad_wide]);
    std::vector<double> gain((size_t)ctx->nch + 3, 1.0);
    if (chain_gain) std::copy(chain_gain, chain_gain + n, gain.begin());
    std::copy(wide, wide + 3, gain.begin() + ctx->nch);
    if (gdg_trim_all_unit(gain.data(), (int)gain.size())) gain.clear();           /* off: as if never called */
    ctx->trim_gain.swap(gain);
    return GDG_OK;
}

/* the delivery factor and the ratio behind it: validated before they replace the ones in force (deliver.h); read by every call that encodes */
static int set_delivery(gdg_ctx *ctx, const char *what, int factor, int up, int down) {
    if (!ctx) return GDG_ERR_INVALID;
    if (ctx->bstream.open) {
        if (gdg_deliver_ratio_on(ctx->deliver_up, ctx->deliver_down))
            return fail(ctx, GDG_ERR_INVALID, "%s: a streamed batch run is open on this context; its delivery factor %d and delivery ratio %d/%d hold until gdg_batch_stream_close", what,
                        ctx->deliver, ctx->deliver_up, ctx->deliver_down);
        return fail(ctx, GDG_ERR_INVALID, "%s: a streamed batch run is open on this context; its delivery factor %d holds until gdg_batch_stream_close", what, ctx->deliver);
    }
    if (!gdg_deliver_factor_ok(factor)) return fail(ctx, GDG_ERR_INVALID, "%s: delivery factor %d; 1 is the session rate, 2 a half of it, 4 a quarter", what, factor);
    if (const int rc = deliver_ratio_check(ctx, what, up, down)) return rc;
    if (factor == ctx->deliver && up == ctx->deliver_up && down == ctx->deliver_down) return GDG_OK;
    std::vector<double> tapsT;
    if (gdg_deliver_ratio_on(up, down)) deliver_ratio_table(up, down, true, tapsT);      /* the prototype, once, in float64 on the host */
    enter(ctx, /*read_only=*/true);                                          /* configuration: no state of the context changes */
    /* another row length: whatever still reads the encoded halves and the scratch rows has to be done before they go -- and a wait that fails
     * refuses the call with the factor in force untouched.  The halves are made anew by the next batch call, at the size of a context that
     * was always configured like this one; back at 1 the scratch rows and the history go as well (the next job with a factor begins from zeros anyway) */
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    batch_drop(ctx, { BATCH_ENCODED, BATCH_DELIVERED, BATCH_DELIVER_HISTORY, BATCH_DELIVER_RATIO_ROWS, BATCH_DELIVER_RATIO_HISTORY, BATCH_DELIVER_RATIO_TABLE });
    ctx->deliver = factor;
    ctx->deliver_up = up;
    ctx->deliver_down = down;
    ctx->deliver_tapsT.swap(tapsT);
    return GDG_OK;
}
int gdg_batch_set_delivery(gdg_ctx *ctx, int factor) { return set_delivery(ctx, "set delivery", factor, 1, 1); }
int gdg_batch_set_out_ratio(gdg_ctx *ctx, int factor, int up, int down) { return set_delivery(ctx, "set delivery ratio", factor, up, down); }

int gdg_batch_delivery(const gdg_ctx *ctx) { return ctx ? ctx->deliver : 1; }
int gdg_batch_delivery_latency(int factor) { return gdg_deliver_latency(factor); }
int gdg_batch_out_ratio(const gdg_ctx *ctx, int *up, int *down) {
    if (up) *up = ctx ? ctx->deliver_up : 1;
    if (down) *down = ctx ? ctx->deliver_down : 1;
    return ctx ? GDG_OK : GDG_ERR_INVALID;
}

/* a shard's master mix is finished elsewhere, from float64 partials at the session rate, and the histories are per context: the shard forms and
 * the finish calls refuse while a factor or a ratio is in force (include/gdg.h) */
static int delivery_refused(gdg_ctx *ctx, const char *what) {
    if (gdg_deliver_ratio_on(ctx->deliver_up, ctx->deliver_down))
        return fail(ctx, GDG_ERR_UNSUPPORTED, "%s: the delivery factor %d with the delivery ratio %d/%d is in force on this context (gdg_batch_set_out_ratio); a sharded job cannot deliver at another rate yet",
                    what, ctx->deliver, ctx->deliver_up, ctx->deliver_down);
    return fail(ctx, GDG_ERR_UNSUPPORTED, "%s: the delivery factor %d is in force on this context (gdg_batch_set_delivery); a sharded job cannot deliver at another rate yet", what, ctx->deliver);
}
#define DELIVERY_REFUSED(ctx, what) delivery_refused(ctx, what)
/* ... and the delivered rows' records are the encoders' rows', with a history per context: the same calls refuse while their switch is on */
#define OUT_RECORDS_REFUSED(ctx, what) \
    fail(ctx, GDG_ERR_UNSUPPORTED, "%s: the delivered rows' records are on on this context (gdg_batch_out_records_enable); a sharded job cannot collect them yet", what)

int gdg_batch_out_records_enable(gdg_ctx *ctx, int enable) {
    if (!ctx) return GDG_ERR_INVALID;
    if (ctx->bstream.open)
        return fail(ctx, GDG_ERR_INVALID, "batch out records: a streamed batch run is open on this context; its setting holds until gdg_batch_stream_close");
    const bool on = enable != 0;
    if (on == ctx->out_rec_on) return GDG_OK;
    enter(ctx, /*read_only=*/true);                                          /* configuration: no state of the context changes */
    /* another size of a download half, and off the history and the spans go: whatever still reads them has to be done first -- a wait that
     * fails refuses the call with the switch untouched.  The halves are made anew by the next batch call, at the size of a context that was
     * always configured like this one. */
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    batch_drop(ctx, { BATCH_ENCODED, BATCH_DELIVERED_REC_HISTORY, BATCH_DELIVERED_REC_SPANS });
    ctx->out_rec_on = on;
    return GDG_OK;
}

/* the blend outputs: validated whole before the list replaces the one in force (blend.h); read when a job is described and by every slice */
int gdg_batch_set_blends_filtered(gdg_ctx *ctx, int n_blends, const int *first, const int *channel, const double *weight, const int *delay, const int *tap_first,
                                  const double *tap, const double *gain) {
    if (!ctx) return GDG_ERR_INVALID;
    if (ctx->bstream.open) return fail(ctx, GDG_ERR_INVALID, "set blends: a streamed batch run is open on this context; its blends hold until gdg_batch_stream_close");
    int b = -1, k = -1, t = -1;
    char msg[240];
    if (const int rc = gdg_blend_check(n_blends, first, channel, weight, delay, gain, ctx->nch, &b, &k)) {
        gdg_blend_list_message(msg, sizeof msg, "set blends", false, rc, b, k, n_blends, first, channel, weight, delay, gain, ctx->nch);
        return fail(ctx, GDG_ERR_INVALID, "%s", msg);
    }
    if (const int rc = gdg_blend_check_taps(n_blends, first, delay, tap_first, tap, &b, &k, &t)) {
        gdg_blend_taps_message(msg, sizeof msg, "set blends", rc, b, k, t, first, delay, tap_first, tap, n_blends);
        return fail(ctx, GDG_ERR_INVALID, "%s", msg);
    }
    enter(ctx, /*read_only=*/true);                                          /* configuration: no state of the context changes */
    const bool resize = n_blends != ctx->blend.count(), had_delay = ctx->blend.max_reach() > 0;
    /* another row count: whatever still reads the window and the encoded halves has to be done before they go -- and a wait that fails
     * refuses the call with the setting in force untouched */
    if (resize || had_delay) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    gdg_blend_replace(ctx->blend, n_blends, first, channel, weight, delay, tap_first, tap, gain, ctx->nch, &b, &k);      /* checked above: it cannot refuse */
    /* no term reaches back any more: the history goes (the next job with one begins from zeros anyway) */
    if (had_delay && ctx->blend.max_reach() == 0) batch_drop(ctx, { BATCH_BLEND_HISTORY });
    if (resize) {
        /* the window and the encoded halves are made anew by the next batch call, at the size of a context that was always configured like
         * this one; off, the table goes as well */
        batch_drop(ctx, { BATCH_WINDOW, BATCH_ENCODED });
        if (ctx->blend.count() == 0) { hipFree(ctx->d_blend); ctx->d_blend = nullptr; ctx->d_blend_cap = 0; }
    }
    return GDG_OK;
}

/* without taps: the filtered call with tap_first == NULL, which takes, packs and uploads the list as it did before taps existed */
int gdg_batch_set_blends_delayed(gdg_ctx *ctx, int n_blends, const int *first, const int *channel, const double *weight, const int *delay, const double *gain) {
    return gdg_batch_set_blends_filtered(ctx, n_blends, first, channel, weight, delay, nullptr, nullptr, gain);
}

int gdg_batch_set_blends(gdg_ctx *ctx, int n_blends, const int *first, const int *channel, const double *weight, const double *gain) {
    return gdg_batch_set_blends_delayed(ctx, n_blends, first, channel, weight, nullptr, gain);
}

int gdg_batch_blends(const gdg_ctx *ctx) { return ctx ? ctx->blend.count() : 0; }
int gdg_batch_blend_max_delay(const gdg_ctx *ctx) { return ctx ? ctx->blend.max_delay() : 0; }
int gdg_batch_blend_max_reach(const gdg_ctx *ctx) { return ctx ? ctx->blend.max_reach() : 0; }

/* Whether taking a new list of kind k drops the last call's records of that kind.  A fit record carries its own term count and stays
 * readable; a Gram, tap-fit or transfer record is read with the list that made it.  (The delivered rows' records have no list to take.) */
static const bool list_enable_drops_records[LIST_DELIVERED] = { false, true, true, true };

/* What the four gdg_batch_*_enable calls that take a list do once it is checked, in front of taking it.  `resized`: the list sends down another
 * size than the one in force -- the download halves are made anew by the next batch call, at the size of a context that was always
 * configured like this one -- whatever still reads them has to be done first -- and off, the table goes as well */
static int list_enable(gdg_ctx *ctx, int k, bool resized) {
    enter(ctx, /*read_only=*/true);                                          /* configuration: no state of the context changes */
    if (resized) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        batch_drop(ctx, { BATCH_ENCODED, BATCH_FIT_TABLE + k });
    }
    if (list_enable_drops_records[k]) ctx->list_rec[k].valid = false;
    return GDG_OK;
}

/* the blend fits: validated whole before the list replaces the one in force (blend.h); the ports' upper bound is the job's, checked when one is described */
int gdg_batch_fit_enable(gdg_ctx *ctx, int n_fits, const int *first, const int *port, const int *target) {
    if (!ctx) return GDG_ERR_INVALID;
    if (ctx->bstream.open) return fail(ctx, GDG_ERR_INVALID, "batch fit: a streamed batch run is open on this context; its fits hold until gdg_batch_stream_close");
    int rc = fit_list_check(ctx, "batch fit", n_fits, first, port, target, -1);            /* the ports' upper bound is the job's */
    if (rc != GDG_OK) return rc;
    if ((rc = list_enable(ctx, LIST_FIT, n_fits != ctx->fit.count())) != GDG_OK) return rc;
    ctx->fit.table = gdg_fit_table(n_fits, first, port, target);
    return GDG_OK;
}

int gdg_batch_fits(const gdg_ctx *ctx) { return ctx ? ctx->fit.count() : 0; }

/* the Gram list: validated whole before it replaces the one in force (blend.h); the ports' upper bound is the job's, checked when one is described */
int gdg_batch_gram_enable(gdg_ctx *ctx, const int *port, int n_ports) {
    if (!ctx) return GDG_ERR_INVALID;
    if (ctx->bstream.open) return fail(ctx, GDG_ERR_INVALID, "batch gram: a streamed batch run is open on this context; its list holds until gdg_batch_stream_close");
    if (n_ports != 0) {
        const int rc = gram_list_check(ctx, "batch gram", port, n_ports, 2, -1);
        if (rc != GDG_OK) return rc;
    }
    const int rc = list_enable(ctx, LIST_GRAM, (size_t)n_ports != ctx->gram_port.size());
    if (rc != GDG_OK) return rc;
    ctx->gram_port.assign(port, port + n_ports);
    return GDG_OK;
}

int gdg_batch_gram_ports(const gdg_ctx *ctx, int *port, int capacity) {
    if (!ctx) return 0;
    const int n = (int)ctx->gram_port.size();
    if (port) for (int i = 0; i < n && i < capacity; i++) port[i] = ctx->gram_port[(size_t)i];
    return n;
}

/* the tap fits: validated whole before they replace the list in force (blend.h); the ports' upper bound is the job's, checked when one is described */
int gdg_batch_tapfit_enable(gdg_ctx *ctx, int n_fits, const int *first, const int *port, const int *target, const int *taps) {
    if (!ctx) return GDG_ERR_INVALID;
    if (ctx->bstream.open) return fail(ctx, GDG_ERR_INVALID, "batch tapfit: a streamed batch run is open on this context; its list holds until gdg_batch_stream_close");
    int rc = tapfit_list_check(ctx, "batch tapfit", n_fits, first, port, target, taps, -1);
    if (rc != GDG_OK) return rc;
    std::vector<int> table = gdg_tapfit_table(n_fits, first, port, target, taps);
    if ((rc = list_enable(ctx, LIST_TAPFIT, table.size() != ctx->tapfit.table.size() || gdg_tapfit_list_doubles(n_fits, first, taps) != ctx->tapfit.doubles())) != GDG_OK) return rc;
    ctx->tapfit.table.swap(table);
    return GDG_OK;
}

int gdg_batch_tapfits(const gdg_ctx *ctx) { return ctx ? ctx->tapfit.count() : 0; }

/* the transfer list: validated whole before it replaces the list in force (blend.h); the ports' upper bound is the job's, checked when one is described */
int gdg_batch_transfer_enable(gdg_ctx *ctx, int n_pairs, const int *port, const int *target, int group) {
    if (!ctx) return GDG_ERR_INVALID;
    if (ctx->bstream.open) return fail(ctx, GDG_ERR_INVALID, "batch transfer: a streamed batch run is open on this context; its list holds until gdg_batch_stream_close");
    if (!port) n_pairs = 0;
    const int rc = transfer_list_check(ctx, "batch transfer", n_pairs, port, target, group, -1);
    if (rc != GDG_OK) return rc;
    static_assert(GDG_TRANSFER_BLOCK == GDG_BLOCK_SIZE, "a block of the batch loop is a block of the transfer record");
    std::vector<int> table = gdg_transfer_table(n_pairs, port, target, group);
    enter(ctx, /*read_only=*/true);                                          /* configuration: no state of the context changes */
    if (n_pairs) {                                                           /* made here: no batch call allocates or uploads the transform's table */
        double2 *tw = nullptr, *tw2 = nullptr;
        const int rt = fir_tables(ctx, GDG_TRANSFER_BLOCK, &tw, &tw2);
        if (rt != GDG_OK) return rt;
    }
    if (const int re = list_enable(ctx, LIST_TRANSFER, gdg_transfer_list_doubles(n_pairs, group) != ctx->transfer.doubles() || table.size() != ctx->transfer.table.size())) return re;
    ctx->transfer.table.swap(table);
    return GDG_OK;
}

int gdg_batch_transfers(const gdg_ctx *ctx) { return ctx ? ctx->transfer.count() : 0; }

/* the master cursor belongs to gdg_batch_finish_master_slice, which is no part of an open job: it may be set while one is open */
int gdg_batch_dither_seek(gdg_ctx *ctx, uint64_t sample_index) {
    if (!ctx) return GDG_ERR_INVALID;
    ctx->dither_cursor = sample_index;
    return GDG_OK;
}

/* a shard's rows are its own channels' and a blend's terms may live on two devices: neither is settled, so the shard calls refuse (include/gdg.h) */
#define BLENDS_REFUSED(ctx, what) \
    fail(ctx, GDG_ERR_UNSUPPORTED, "%s: %d blends are in force on this context (gdg_batch_set_blends); a sharded job cannot write blend outputs yet", what, (ctx)->blend.count())

/* ... and a fit's, a Gram list's, a tap fit's and a transfer pair's ports are rows of the one-device window: the same refusal, the first kind in
 * force in its own words -- the four kinds that have a list; the delivered rows' records refuse in theirs (OUT_RECORDS_REFUSED) */
int lists_refused(gdg_ctx *ctx, const char *what) {
    static const char *const text[LIST_DELIVERED] = {
        "%s: %d fits are in force on this context (gdg_batch_fit_enable); a sharded job cannot collect fit records yet",
        "%s: a Gram list of %d ports is in force on this context (gdg_batch_gram_enable); a sharded job cannot collect Gram records yet",
        "%s: %d tap fits are in force on this context (gdg_batch_tapfit_enable); a sharded job cannot collect tap-fit records yet",
        "%s: %d transfer pairs are in force on this context (gdg_batch_transfer_enable); a sharded job cannot collect transfer records yet" };
    for (int k = 0; ctx && k < LIST_DELIVERED; k++) {
        const int count = list_in_force(ctx, k, 0).count;
        if (count) return fail(ctx, GDG_ERR_UNSUPPORTED, text[k], what, count);
    }
    return GDG_OK;
}

#define SHARD_PORTS " (a shard: its N inputs, its N outputs, metronome, left, right)"
static int check_meter_ports(gdg_ctx *ctx, const gdg_batch_options *opt, const char *note) {
    if (opt->run_meters && ctx->n_meter != 2 * ctx->nch + 3)
        return fail(ctx, GDG_ERR_INVALID, "level meters: %d ports configured, the batch needs 2 N + 3 = %d%s", ctx->n_meter, 2 * ctx->nch + 3, note);
    return GDG_OK;
}

/* The one description of a batch job: inputs and options validated, every input's covered samples, the job's padded length.
 * `shard`: the job of gdg_batch_run_shard (job_samples, run_metronome) instead of gdg_batch_run's.  `meters_at_open`: a job that stays
 * open refuses at once what each of its slices would refuse; the one-call run checks its ports itself, behind its empty job's early end. */
int stream_job(gdg_ctx *ctx, const gdg_batch_input *inputs, int n_inputs, const gdg_batch_options *opt, bool shard, size_t job_samples,
               bool run_metronome, gdg_ctx::BatchStreamState &S, bool meters_at_open) {
    if (!ctx || !inputs || !opt) return GDG_ERR_INVALID;
    if (ctx->bstream.open) return fail(ctx, GDG_ERR_INVALID, "a streamed batch run is already open on this context");
    if (n_inputs != ctx->nch) return fail(ctx, GDG_ERR_INVALID, "the batch has %d inputs, the context %d channels", n_inputs, ctx->nch);
    if (ctx->max_frames < GDG_BLOCK_SIZE)
        return fail(ctx, GDG_ERR_INVALID, "the batch loop runs blocks of %d frames, the context allows %d", GDG_BLOCK_SIZE, ctx->max_frames);
    if (!gdg_wave_bytes_per_sample(opt->out_format)) return fail(ctx, GDG_ERR_UNSUPPORTED, "unknown sample format %d", opt->out_format);
    if (opt->target_rate == 0) return fail(ctx, GDG_ERR_INVALID, "sample rate must be positive");
    const int n_blends = shard ? 0 : ctx->blend.count();                         /* the shard calls refuse blends before they come here */
    if (!ctx->align_ref.empty() && (int)ctx->align_ref.size() != n_inputs + (shard ? 1 : 3) && (n_blends == 0 || (int)ctx->align_ref.size() != n_inputs + 3 + n_blends)) {      /* before anything is done */
        if (n_blends)
            return fail(ctx, GDG_ERR_INVALID, "batch align: the list in force has %zu ports, this call %d (the N chain outputs, master left, master right, metronome) or %d "
                        "(those and the %d blends in force)", ctx->align_ref.size(), n_inputs + 3, n_inputs + 3 + n_blends, n_blends);
        return fail(ctx, GDG_ERR_INVALID, "batch align: the list in force has %zu ports, this call %d (%s)", ctx->align_ref.size(), n_inputs + (shard ? 1 : 3),
                    shard ? "a shard's n chain outputs and the metronome" : "the N chain outputs, master left, master right, metronome");
    }
    if (n_blends && ctx->dither_mode != 0 && !gdg_dither_ports_ok(ctx->dither_port_base, n_inputs + 3 + n_blends))
        return fail(ctx, GDG_ERR_INVALID, "blends: the dither's port_base %u + %d channels + 3 + %d blends reaches the job-wide ports from 0x%x on", ctx->dither_port_base,
                    n_inputs, n_blends, GDG_DITHER_PORT_MASTER_LEFT);
    if (!shard && ctx->fit.count()) {                                            /* the fits' ports against this call's: the shard calls refuse fits before they come here */
        int term = -1;
        const int f = ctx->fit.first_outside(n_inputs + 3 + n_blends, &term);
        if (f >= 0 && term < 0)
            return fail(ctx, GDG_ERR_INVALID, "batch fit: fit %d has the target port %d, this call has ports 0 to %d (N + 3 = %d and %d blends)", f, ctx->fit.target(f),
                        n_inputs + 2 + n_blends, n_inputs + 3, n_blends);
        if (f >= 0)
            return fail(ctx, GDG_ERR_INVALID, "batch fit: fit %d, term %d names port %d, this call has ports 0 to %d (N + 3 = %d and %d blends)", f, term, ctx->fit.port(f, term),
                        n_inputs + 2 + n_blends, n_inputs + 3, n_blends);
    }
    if (!shard && !ctx->gram_port.empty()) {                                     /* the list's ports against this call's */
        const int at = gdg_gram_list_bad(ctx->gram_port.data(), (int)ctx->gram_port.size(), n_inputs + 3 + n_blends);
        if (at >= 0)
            return fail(ctx, GDG_ERR_INVALID, "batch gram: list entry %d names port %d, this call has ports 0 to %d (N + 3 = %d and %d blends)", at, ctx->gram_port[(size_t)at],
                        n_inputs + 2 + n_blends, n_inputs + 3, n_blends);
    }
    if (!shard && ctx->tapfit.count()) {                                         /* the tap fits' ports against this call's */
        int term = -1;
        const int f = ctx->tapfit.first_outside(n_inputs + 3 + n_blends, &term);
        if (f >= 0 && term < 0)
            return fail(ctx, GDG_ERR_INVALID, "batch tapfit: fit %d has the target port %d, this call has ports 0 to %d (N + 3 = %d and %d blends)", f, ctx->tapfit.target(f),
                        n_inputs + 2 + n_blends, n_inputs + 3, n_blends);
        if (f >= 0)
            return fail(ctx, GDG_ERR_INVALID, "batch tapfit: fit %d, term %d names port %d, this call has ports 0 to %d (N + 3 = %d and %d blends)", f, term, ctx->tapfit.port(f, term),
                        n_inputs + 2 + n_blends, n_inputs + 3, n_blends);
    }
    if (!shard && ctx->transfer.count()) {                                       /* the transfer pairs' ports against this call's */
        int side = 0;
        const int q = ctx->transfer.first_outside(n_inputs + 3 + n_blends, &side);
        if (q >= 0)
            return fail(ctx, GDG_ERR_INVALID, "batch transfer: pair %d has the %s port %d, this call has ports 0 to %d (N + 3 = %d and %d blends)", q, side ? "target" : "measured",
                        side ? ctx->transfer.target(q) : ctx->transfer.port(q), n_inputs + 2 + n_blends, n_inputs + 3, n_blends);
    }
    int rc;
    if (meters_at_open && (rc = check_meter_ports(ctx, opt, shard ? SHARD_PORTS : "")) != GDG_OK) return rc;
    std::vector<size_t> n_out((size_t)n_inputs, 0);
    size_t max_len = 0;
    /* a source map with a reader (gdg_batch_set_sources): only the roots' entries are looked at, and the job's length is theirs */
    const bool shared = batch_sources_shared(ctx);
    for (int i = 0; i < n_inputs; i++) {
        const gdg_batch_input &in = inputs[i];
        if (shared && ctx->batch_source[(size_t)i] != i) continue;
        if (!in.bytes || !in.samples_per_channel) continue;
        if (!gdg_wave_bytes_per_sample(in.format)) return fail(ctx, GDG_ERR_UNSUPPORTED, "input %d: unknown sample format %d", i, in.format);
        if (in.channels == 0 || in.channel >= in.channels) return fail(ctx, GDG_ERR_INVALID, "input %d: channel %u of %u", i, in.channel, in.channels);
        if (in.sample_rate == 0) return fail(ctx, GDG_ERR_INVALID, "input %d: sample rate must be positive", i);
        n_out[(size_t)i] = input_covers(in, opt->target_rate);
        max_len = std::max(max_len, n_out[(size_t)i]);
    }
    max_len = whole_blocks(max_len);
    if (shard && job_samples) {                                                  /* the shard pads to the job's length, as gdg_batch_run_shard does */
        if (job_samples < max_len || job_samples % GDG_BLOCK_SIZE)
            return fail(ctx, GDG_ERR_INVALID, "the job's %zu samples: at least this shard's %zu and a multiple of %d", job_samples, max_len, GDG_BLOCK_SIZE);
        max_len = job_samples;
    }
    S.shard = shard;
    S.run_metro = shard ? run_metronome : true;
    S.inputs.assign(inputs, inputs + n_inputs);
    S.source.clear();
    if (shared) {                                                                /* a reader: metadata, length and empty-or-not of its root */
        S.source = ctx->batch_source;
        for (int i = 0; i < n_inputs; i++) {
            const size_t root = (size_t)S.source[(size_t)i];
            if (root == (size_t)i) continue;
            S.inputs[(size_t)i] = inputs[root];
            n_out[(size_t)i] = n_out[root];
        }
    }
    S.opt = *opt;
    S.length = max_len;
    S.pos = 0;
    S.brought.assign((size_t)n_inputs, 0);
    S.n_out = n_out;
    S.open = true;
    return GDG_OK;
}

static int stream_open(gdg_ctx *ctx, const gdg_batch_input *inputs, int n_inputs, const gdg_batch_options *opt, bool shard, size_t job_samples,
                       bool run_metronome, size_t *samples) {
    if (!ctx || !samples) return GDG_ERR_INVALID;
    gdg_ctx::BatchStreamState job;
    const int rc = stream_job(ctx, inputs, n_inputs, opt, shard, job_samples, run_metronome, job);
    if (rc != GDG_OK) return rc;
    ctx->bstream = job;
    *samples = job.length;
    return GDG_OK;
}

int gdg_batch_stream_open(gdg_ctx *ctx, const gdg_batch_input *inputs, int n_inputs, const gdg_batch_options *opt, size_t *samples) {
    return stream_open(ctx, inputs, n_inputs, opt, false, 0, true, samples);
}

int gdg_batch_stream_open_shard(gdg_ctx *ctx, const gdg_batch_input *inputs, int n_inputs, const gdg_batch_options *opt, size_t job_samples,
                                int run_metronome, size_t *samples) {
    if (ctx && delivery_on(ctx)) return DELIVERY_REFUSED(ctx, "gdg_batch_stream_open_shard");
    if (ctx && ctx->out_rec_on) return OUT_RECORDS_REFUSED(ctx, "gdg_batch_stream_open_shard");
    if (const int rl = loudness_refused(ctx, "gdg_batch_stream_open_shard", "a sharded job cannot collect them yet")) return rl;
    if (ctx && ctx->blend.count()) return BLENDS_REFUSED(ctx, "gdg_batch_stream_open_shard");
    if (const int rc = lists_refused(ctx, "gdg_batch_stream_open_shard")) return rc;
    /* as gdg_batch_run_shard: a set flag would be silently dropped -- refuse it instead */
    if (ctx && opt && opt->metronome_to_master)
        return fail(ctx, GDG_ERR_INVALID, "gdg_batch_stream_open_shard: metronome_to_master must be 0 -- a shard's master mix is a partial sum; pass the metronome's "
                    "float64 track (gdg_batch_shard_out.metronome of the shard that runs it) as `aux` to gdg_batch_finish_master_slice");
    return stream_open(ctx, inputs, n_inputs, opt, true, job_samples, run_metronome != 0, samples);
}

/* the source frames [first, first + count) of every input that the job's samples [pos, pos + blocks * 8192) bring */
static void stream_need(const gdg_ctx::BatchStreamState &S, size_t out_count, size_t *first, size_t *count) {
    for (size_t i = 0; i < S.inputs.size(); i++) {
        const gdg_batch_input &in = S.inputs[i];
        first[i] = S.brought[i];
        count[i] = 0;
        if (!in.bytes || !in.samples_per_channel) continue;
        size_t sf = 0, sc = 0;
        gdg_batch_stream_span(in.samples_per_channel, in.sample_rate, S.opt.target_rate, S.pos, out_count, &sf, &sc);
        if (sc && sf + sc > S.brought[i]) count[i] = sf + sc - S.brought[i];
    }
    for (size_t i = 0; i < S.source.size(); i++)                                 /* a reader brings nothing: its frames are its root's */
        if (S.source[i] != (int)i) { first[i] = first[(size_t)S.source[i]]; count[i] = 0; }
}

static int stream_check_blocks(gdg_ctx *ctx, int blocks) {
    const auto &S = ctx->bstream;
    if (!S.open) return fail(ctx, GDG_ERR_INVALID, "no streamed batch run is open on this context");
    if (S.pos >= S.length) return fail(ctx, GDG_ERR_INVALID, "the streamed batch run has delivered its last block");
    if (blocks < 1 || (size_t)blocks > (S.length - S.pos) / GDG_BLOCK_SIZE)
        return fail(ctx, GDG_ERR_INVALID, "a slice of %d blocks: 1 to the %zu blocks left of the job", blocks, (S.length - S.pos) / GDG_BLOCK_SIZE);
    if ((size_t)blocks * GDG_BLOCK_SIZE > 0x7fffffff) return fail(ctx, GDG_ERR_INVALID, "a slice of %d blocks is too long", blocks);
    return GDG_OK;
}

int gdg_batch_stream_need(gdg_ctx *ctx, int blocks, size_t *first, size_t *count) {
    if (!ctx || !first || !count) return GDG_ERR_INVALID;
    const int rc = stream_check_blocks(ctx, blocks);
    if (rc != GDG_OK) return rc;
    stream_need(ctx->bstream, (size_t)blocks * GDG_BLOCK_SIZE, first, count);
    return GDG_OK;
}

int gdg_batch_stream_close(gdg_ctx *ctx) {
    if (!ctx) return GDG_ERR_INVALID;
    if (!ctx->bstream.open) return fail(ctx, GDG_ERR_INVALID, "no streamed batch run is open on this context");
    ctx->bstream.open = false;                 /* the buffers stay with the context (gdg_batch_release) */
    return GDG_OK;
}

/* a job with shared sources: channel c reads another channel's input (its root's piece is stored to its row as well) */
static bool is_reader(const gdg_ctx::BatchStreamState &S, int c) { return !S.source.empty() && S.source[(size_t)c] != c; }

/* What ONE STEP (at most W blocks) can bring per input, and the halves that hold it: the sizes depend on the window, not on the slice or the
 * job.  An upload half: the descriptors -- a piece and a carry per input; with shared sources the descriptors are the fan-out forms (a step
 * without a reader writes the plain ones into the same room) and a table of the rows they name follows: every channel's row once, two
 * source-buffer rows per resampled root -- then the inputs' pieces.  A source half: the resampled inputs' frames. */
namespace {                                     /* nothing of the upload side leaves this file */
struct UploadLayout {
    std::vector<size_t> cap, src_off;
    std::vector<double> dx;
    size_t dec_rows_bytes, spans_bytes, table_bytes, up_rows_bytes, up_half, src_half;
    bool any;                                   /* some input has samples */
};

static UploadLayout upload_layout(const gdg_ctx::BatchStreamState &S, int N, size_t ws) {
    const bool shared = !S.source.empty();
    UploadLayout L = { std::vector<size_t>((size_t)N, 0), std::vector<size_t>((size_t)N, 0), std::vector<double>((size_t)N, 1.0), 0, 0, 0, 0, 0, 0, false };
    L.dec_rows_bytes = ((size_t)2 * N * (shared ? sizeof(gdg_decode_fan) : sizeof(gdg_decode_row)) + 255) & ~(size_t)255;
    L.spans_bytes = ((size_t)N * (shared ? sizeof(gdg_resample_fan) : sizeof(gdg_resample_span)) + 255) & ~(size_t)255;
    L.table_bytes = shared ? ((size_t)3 * N * sizeof(double *) + 255) & ~(size_t)255 : 0;
    L.up_half = L.up_rows_bytes = L.dec_rows_bytes + L.spans_bytes + L.table_bytes;
    for (int i = 0; i < N; i++) {
        const gdg_batch_input &in = S.inputs[(size_t)i];
        if (!in.bytes || !in.samples_per_channel) continue;
        L.any = true;
        if (is_reader(S, i)) continue;                                           /* only roots size the upload halves and the source halves */
        L.cap[(size_t)i] = ws;
        if (in.sample_rate != S.opt.target_rate) {
            L.dx[(size_t)i] = (double)in.sample_rate / (double)S.opt.target_rate;
            L.cap[(size_t)i] = (size_t)((double)ws * L.dx[(size_t)i]) + 16;
            L.src_off[(size_t)i] = L.src_half;
            L.src_half += ((L.cap[(size_t)i] + GDG_STREAM_CARRY) * sizeof(double) + 15) & ~(size_t)15;
        }
        L.up_half += (L.cap[(size_t)i] * in.channels * (size_t)gdg_wave_bytes_per_sample(in.format) + 15) & ~(size_t)15;
    }
    L.up_half = (L.up_half + 255) & ~(size_t)255;                               /* the second half starts with descriptors: aligned like the first */
    L.src_half = (L.src_half + 255) & ~(size_t)255;
    return L;
}

/* One step's upload while it is put together in its pinned half: the plain descriptors where they go; with shared sources the fan-out forms,
 * made aside and written into the half once the step is known to have a reader (or not: then as the plain descriptors, for the kernels every
 * other job runs), and the table of the rows they name; the host pieces to move, and how far the half is filled */
struct StepUpload {
    gdg_decode_row *rows;
    gdg_resample_span *spans;
    size_t cur;
    std::vector<gdg_decode_fan> dfans;
    std::vector<gdg_resample_fan> rfans;
    std::vector<double *> table;
    std::vector<BatchPiece> pieces;
    bool step_fans = false;
    int n_rows = 0, n_spans = 0;
    unsigned max_count = 0, max_out = 0;
};

/* The upload side of a slice (BatchStage): step i's inputs, the loop's samples [a, a + w * 8192), gathered into pinned half i & 1, moved and
 * decoded -- and resampled -- on the upload stream.  It keeps, from step to step, which halves are in use and the frames handed over. */
struct SliceStage {
    gdg_ctx *ctx;
    const gdg_ctx::BatchStreamState &S;
    const void *const *in_bytes;
    const UploadLayout &L;
    const SourceFans &fans;
    const std::vector<size_t> &first, &count;   /* the frames the slice brings per input (stream_need) */
    size_t length, pos;
    double *d_inputs, *d_carry;
    unsigned char *d_up, *d_src;
    std::vector<size_t> run;                    /* frames handed over, step by step */
    int up_used[2];

    /* the rows root c feeds in this step into the table: `own` (its row, or its place in the source buffer), then its readers' rows */
    void fan_rows(StepUpload &u, double *own, int c, size_t a, bool with_readers, unsigned *dst_first, unsigned *n_dst, unsigned *vec) const {
        *dst_first = (unsigned)u.table.size();
        u.table.push_back(own);
        if (with_readers)
            for (int k = 0; k < fans.fan(c); k++) u.table.push_back(d_inputs + (size_t)fans.readers(c)[k] * length + a);
        *n_dst = (unsigned)u.table.size() - *dst_first;
        *vec = 1;
        for (size_t k = *dst_first; k < u.table.size(); k++) if ((uintptr_t)u.table[k] & 15) *vec = 0;
        if (*n_dst > 1) u.step_fans = true;
    }
    void put_row(StepUpload &u, const unsigned char *src, double *dst, int c, size_t a, bool with_readers, unsigned cnt, int fmt, unsigned stride, unsigned offset) const {
        if (S.source.empty()) { u.rows[u.n_rows++] = gdg_decode_row{ src, dst, cnt, fmt, stride, offset }; return; }
        gdg_decode_fan f = { src, cnt, fmt, stride, offset, 0, 0, 0, 0 };
        fan_rows(u, dst, c, a, with_readers, &f.dst_first, &f.n_dst, &f.vec);
        u.dfans.push_back(f);
        u.n_rows++;
    }

    /* input c's part of the step [a, a + span) in half h: its fresh frames as host pieces, its decode rows and, at another rate, its span */
    int input(StepUpload &u, int c, int h, size_t a, size_t span) {
        const gdg_batch_input &in = S.inputs[(size_t)c];
        const uint32_t rate = S.opt.target_rate;
        const size_t abs = pos + a;                                          /* the step: the job's samples [abs, abs + span) */
        if (is_reader(S, c)) return GDG_OK;                                  /* its root's piece is stored to its row as well */
        if (!in.bytes || !in.samples_per_channel || abs >= S.n_out[(size_t)c]) return GDG_OK;      /* empty, or ended in an earlier step: zeros */
        unsigned char *hb = ctx->h_up[h], *db = d_up + (size_t)h * L.up_half, *sb = d_src + (size_t)h * L.src_half;
        const size_t cnt = std::min(S.n_out[(size_t)c] - abs, span), width = (size_t)gdg_wave_bytes_per_sample(in.format) * in.channels;
        size_t sf = 0, sc = 0;
        gdg_batch_stream_span(in.samples_per_channel, in.sample_rate, rate, abs, cnt, &sf, &sc);
        const size_t bs = run[(size_t)c], e = std::max(bs, sf + sc), fresh = e - bs;
        if (fresh > L.cap[(size_t)c] || bs < first[(size_t)c] || e > first[(size_t)c] + count[(size_t)c])
            return fail(ctx, GDG_ERR_INVALID, "input %d: a step of %zu frames from %zu does not fit its slice", c, fresh, bs);
        run[(size_t)c] = e;
        const unsigned char *src = static_cast<const unsigned char *>(in_bytes[c]) + (bs - first[(size_t)c]) * width;
        const unsigned stride = in.channels > 1 ? in.channels : 0;
        double *row = d_inputs + (size_t)c * length + a;
        unsigned char *piece = db + u.cur;
        if (fresh) {
            for (size_t q = 0; q < fresh * width; q += (size_t)1 << 20)
                u.pieces.push_back({ hb + u.cur + q, src + q, std::min(fresh * width - q, (size_t)1 << 20) });
            u.cur += (fresh * width + 15) & ~(size_t)15;
            if (fresh > u.max_count) u.max_count = (unsigned)fresh;
            ctx->batch_up_bytes += fresh * width;
        }
        if (in.sample_rate == rate) {
            if (bs != abs || fresh != cnt) return fail(ctx, GDG_ERR_INVALID, "input %d: step at %zu, frames from %zu", c, abs, bs);
            put_row(u, piece, row, c, a, true, (unsigned)cnt, in.format, stride, in.channel);
            return GDG_OK;
        }
        /* resample.Time: [the frames kept from the step before | this step's], then the span kernel */
        const size_t keep_in = std::min(bs, (size_t)GDG_STREAM_CARRY), held = keep_in + fresh;
        if (sf < bs - keep_in) return fail(ctx, GDG_ERR_INVALID, "input %d: the resampler looks back to frame %zu, kept from %zu", c, sf, bs - keep_in);
        double *frames = reinterpret_cast<double *>(sb + L.src_off[(size_t)c]), *carry = d_carry + (size_t)c * GDG_STREAM_CARRY;
        if (keep_in) put_row(u, reinterpret_cast<const unsigned char *>(carry), frames, c, a, false, (unsigned)keep_in, GDG_FMT_IEEE64, 0, 0);
        if (fresh) put_row(u, piece, frames + keep_in, c, a, false, (unsigned)fresh, in.format, stride, in.channel);
        if (keep_in > u.max_count) u.max_count = (unsigned)keep_in;
        const gdg_resample_span sp = { frames, row, carry, (long long)(bs - keep_in), (long long)in.samples_per_channel, (long long)abs,
                                       L.dx[(size_t)c], (unsigned)cnt, (unsigned)held, (unsigned)std::min(held, (size_t)GDG_STREAM_CARRY), 0 };
        if (S.source.empty()) u.spans[u.n_spans++] = sp;
        else {
            gdg_resample_fan f = { sp, 0, 0 };
            unsigned vec = 0;
            fan_rows(u, row, c, a, true, &f.dst_first, &f.n_dst, &vec);
            u.rfans.push_back(f);
            u.n_spans++;
        }
        ctx->batch_resampled += cnt;
        if (cnt > u.max_out) u.max_out = (unsigned)cnt;
        return GDG_OK;
    }

    /* the step put together: its descriptors written, its pieces moved into the pinned half, the half sent up, decode and resample launched */
    int send(StepUpload &u, int h, int pool) {
        unsigned char *hb = ctx->h_up[h], *db = d_up + (size_t)h * L.up_half;
        if (!S.source.empty() && u.n_rows) {
            if (u.table.size() * sizeof(double *) > L.table_bytes) return fail(ctx, GDG_ERR_INVALID, "a step names %zu rows, its table holds %d", u.table.size(), 3 * ctx->nch);
            if (u.step_fans) {
                memcpy(hb, u.dfans.data(), u.dfans.size() * sizeof(gdg_decode_fan));
                if (u.n_spans) memcpy(hb + L.dec_rows_bytes, u.rfans.data(), u.rfans.size() * sizeof(gdg_resample_fan));
                memcpy(hb + L.dec_rows_bytes + L.spans_bytes, u.table.data(), u.table.size() * sizeof(double *));
            } else {                                                         /* no reader in this step: every fan is its first row */
                for (size_t k = 0; k < u.dfans.size(); k++)
                    u.rows[k] = gdg_decode_row{ u.dfans[k].src, u.table[u.dfans[k].dst_first], u.dfans[k].count, u.dfans[k].fmt, u.dfans[k].stride, u.dfans[k].offset };
                for (size_t k = 0; k < u.rfans.size(); k++) u.spans[k] = u.rfans[k].span;
            }
        }
        if (u.n_rows) {
            move_pieces(ctx, u.pieces, pool);
            HIP_TRY(ctx, hipMemcpyAsync(db, hb, u.cur, hipMemcpyHostToDevice, ctx->batch_up_stream));
            if (u.step_fans) {
                /* the fan-out launches: a root's piece decoded once, its span resampled once, stored to every row of its fan */
                double *const *d_table = reinterpret_cast<double *const *>(db + L.dec_rows_bytes + L.spans_bytes);
                HIP_TRY(ctx, gdg_launch_wave_decode_fans(reinterpret_cast<const gdg_decode_fan *>(db), d_table, u.n_rows, u.max_count, ctx->batch_up_stream));
                HIP_TRY(ctx, gdg_launch_resample_fans(reinterpret_cast<const gdg_resample_fan *>(db + L.dec_rows_bytes), d_table, u.n_spans, u.max_out, ctx->batch_up_stream));
            } else {
                /* ONE decode launch for every piece and every kept frame, ONE resample launch for every resampled input */
                HIP_TRY(ctx, gdg_launch_wave_decode_rows(reinterpret_cast<const gdg_decode_row *>(db), u.n_rows, u.max_count, ctx->batch_up_stream));
                HIP_TRY(ctx, gdg_launch_resample_spans(reinterpret_cast<const gdg_resample_span *>(db + L.dec_rows_bytes), u.n_spans, u.max_out, ctx->batch_up_stream));
            }
        }
        HIP_TRY(ctx, hipEventRecord(ctx->batch_up_ready[h], ctx->batch_up_stream));
        return GDG_OK;
    }

    int operator()(size_t i, size_t a, int w, int pool) {
        const int h = (int)(i & 1);
        if (up_used[h]) HIP_TRY(ctx, hipEventSynchronize(ctx->batch_up_ready[h]));     /* step i - 2 has left this half */
        StepUpload u = { reinterpret_cast<gdg_decode_row *>(ctx->h_up[h]), reinterpret_cast<gdg_resample_span *>(ctx->h_up[h] + L.dec_rows_bytes), L.up_rows_bytes };
        for (int c = 0; c < ctx->nch; c++)
            if (const int r = input(u, c, h, a, (size_t)w * GDG_BLOCK_SIZE)) return r;
        up_used[h] = 1;
        return send(u, h, pool);
    }
};
}

/* The settings in force go up, and `loop` gets what they need on the device: the list records' tables, the trim, the blends, the delivery, the
 * ratio behind it and the delivered records' buffers of a slice of `blocks` blocks at the job's sample `pos`.  n_blends, R, RL / RM: the
 * blends, the delivery factor and the ratio in force -- never a shard's. */
static int slice_settings(gdg_ctx *ctx, const ListInForce *lists, int n_blends, int R, int RL, int RM, size_t pos, int blocks, BatchLoop &loop) {
    const int N = ctx->nch, NO = N + 3, NR = NO + n_blends;
    const size_t ws = loop.ws;
    int r;
    /* the list records in force.  A kind with a table -- the fits', the Gram list, the tap fits', the transfer list's: it goes up into the
     * kind's slot on the context's stream, ahead of everything the slice enqueues there; it lives as long as the setting, so nothing waits here */
    for (int k = 0; k < LIST_KINDS; k++) {
        const ListInForce &L = lists[k];
        if (!L.count) continue;
        int *d_table = nullptr;
        if (L.ints > 0) {
            if ((r = batch_buffer(ctx, BATCH_FIT_TABLE + k, L.ints * sizeof(int), (void **)&d_table)) != GDG_OK) return r;
            HIP_TRY(ctx, hipMemcpyAsync(d_table, L.table, L.ints * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        }
        loop.list[k] = { L.table, d_table, L.count, L.shape };
    }
    /* the trim in force: its N + 3 gains go up on the context's stream, ahead of everything the slice enqueues there */
    if (!ctx->trim_gain.empty()) {
        if (!ctx->d_trim && hipMalloc((void **)&ctx->d_trim, (size_t)NO * sizeof(double)) != hipSuccess)
            return fail(ctx, GDG_ERR_NOMEM, "the batch run cannot allocate the trim's %d gains on the device", NO);
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_trim, ctx->trim_gain.data(), (size_t)NO * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        loop.d_trim = ctx->d_trim;
    }
    /* the blends in force: their table goes up the same way, as it was packed when the list was taken (blend.h, gdg_blend_pack) */
    if (n_blends) {
        const BlendSet &bs = ctx->blend;                                      /* it lives as long as the setting, so nothing waits here */
        const size_t bytes = bs.packed.size();
        if (bytes > ctx->d_blend_cap) {
            hipFree(ctx->d_blend);
            ctx->d_blend = nullptr;
            ctx->d_blend_cap = 0;
            if (hipMalloc((void **)&ctx->d_blend, bytes) != hipSuccess) return fail(ctx, GDG_ERR_NOMEM, "the batch run cannot allocate the table of %d blends on the device", n_blends);
            ctx->d_blend_cap = bytes;
        }
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_blend, bs.packed.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
        loop.n_blends = n_blends;
        loop.blend = bs.view(ctx->d_blend);
        loop.d_blend_gain = bs.unit_gains() ? nullptr : loop.blend.gain;
        if (bs.max_reach() > 0) {
            /* the history of the N chain rows: the job's first slice begins from zeros, every later one from what the slice before left */
            if ((r = carried_history(ctx, BATCH_BLEND_HISTORY, (size_t)N * GDG_BLEND_MAX_DELAY * sizeof(double), pos, "blend", &loop.d_blend_history)) != GDG_OK) return r;
        }
    }
    /* the delivery in force: the scratch rows the encoders read, and the history of the window's NR rows -- the job's first slice begins from
     * zeros, every later one from what the slice before left */
    if (R > 1) {
        if ((r = batch_buffer(ctx, BATCH_DELIVERED, (size_t)NR * (ws / (size_t)R) * sizeof(double), (void **)&loop.d_delivered)) != GDG_OK) return r;
        if ((r = carried_history(ctx, BATCH_DELIVER_HISTORY, (size_t)NR * GDG_DELIVER_HISTORY * sizeof(double), pos, "delivery", &loop.d_deliver_history)) != GDG_OK) return r;
        loop.deliver = R;
        loop.d_deliver_taps = R == 2 ? ctx->os.taps2 : ctx->os.taps4;           /* the oversampler's expanded tables (api_ctx.cpp) */
    }
    /* ... and the ratio behind it: the rows the encoders then read, at the window's fixed pitch; the table, which goes up ahead of everything the
     * slice enqueues; the history of the NR intermediate rows, zeroed by the job's first slice like the factor's */
    if (gdg_deliver_ratio_on(RL, RM)) {
        const size_t table_bytes = ctx->deliver_tapsT.size() * sizeof(double);
        double *d_table = nullptr;
        loop.ratio_stride = gdg_deliver_pitch(R, RL, RM, ws);
        if ((r = batch_buffer(ctx, BATCH_DELIVER_RATIO_ROWS, (size_t)NR * loop.ratio_stride * sizeof(double), (void **)&loop.d_ratio_rows)) != GDG_OK) return r;
        if ((r = batch_buffer(ctx, BATCH_DELIVER_RATIO_TABLE, table_bytes, (void **)&d_table)) != GDG_OK) return r;
        if ((r = carried_history(ctx, BATCH_DELIVER_RATIO_HISTORY, (size_t)NR * GDG_DELIVER_RATIO_HISTORY * sizeof(double), pos, "delivery ratio's", &loop.d_ratio_history)) != GDG_OK) return r;
        HIP_TRY(ctx, hipMemcpyAsync(d_table, ctx->deliver_tapsT.data(), table_bytes, hipMemcpyHostToDevice, ctx->stream));
        loop.ratio_up = RL;
        loop.ratio_down = RM;
        loop.d_ratio_taps = d_table;
    }
    /* the delivered rows' records: the history of the NR rows the encoders read, zeroed by the job's first slice like the deliveries'; room for
     * the spans of the slice's steps -- a step has w + 1 of them, so never more than two per block */
    if (lists[LIST_DELIVERED].count) {
        if ((r = batch_buffer(ctx, BATCH_DELIVERED_REC_SPANS, (size_t)2 * (size_t)blocks * sizeof(unsigned long long), (void **)&loop.d_out_rec_spans)) != GDG_OK) return r;
        if ((r = carried_history(ctx, BATCH_DELIVERED_REC_HISTORY, (size_t)NR * GDG_OUT_RECORDS_HISTORY * sizeof(double), pos, "delivered rows'", &loop.d_out_rec_history)) != GDG_OK) return r;
    }
    return GDG_OK;
}

/* The slice runner: the job's samples [S.pos, S.pos + blocks * 8192), which the caller has checked to lie in the job; `slice`: the partial
 * master and metronome buffers of a shard's job, null for any other.  The job is the caller's (an open one of the context, or the
 * one-call run's own) and is left as it is: `brought` gets what the caller commits with S.pos once the slice has run.  `begun`: the
 * slice got as far as the device -- a failure from there on leaves units and meters part-way through it. */
static int run_slice(gdg_ctx *ctx, const gdg_ctx::BatchStreamState &S, int blocks, const void *const *in_bytes, void *const *out_bytes,
                     const gdg_batch_shard_out *slice, std::vector<size_t> &brought, bool &begun) {
    begun = false;
    const bool sharded = S.shard;
    const gdg_batch_options *opt = &S.opt;
    const int N = ctx->nch, NO = N + 3, B = GDG_BLOCK_SIZE, out_width = gdg_wave_bytes_per_sample(opt->out_format);
    const size_t length = (size_t)blocks * B, pos = S.pos;                       /* the slice: rows of `length` samples, the job's [pos, pos + length) */
    /* the blends in force (never a shard's): NR rows of the window leave the device encoded, and every record kind has NR ports */
    const int n_blends = sharded ? 0 : ctx->blend.count(), NR = NO + n_blends;
    const int R = sharded ? 1 : ctx->deliver;                                    /* the delivery factor in force (never a shard's: its calls refuse it) */
    const int RL = sharded ? 1 : ctx->deliver_up, RM = sharded ? 1 : ctx->deliver_down;      /* ... and the ratio behind it */
    report_begin(ctx, sharded ? N + 1 : NR, (size_t)blocks, true, n_blends);
    ListInForce lists[LIST_KINDS];                                               /* the list records in force; never a shard's: its calls refuse them */
    ListShape list_shape[LIST_KINDS];
    for (int k = 0; k < LIST_KINDS; k++) {
        lists[k] = sharded ? ListInForce{ nullptr, 0, 0, { 0, 0 } } : list_in_force(ctx, k, NR);
        list_shape[k] = lists[k].shape;
        if (lists[k].count) list_begin(ctx, k, (size_t)blocks, NR);
    }
    ctx->batch_up_bytes = ctx->batch_resampled = 0;
    /* a job with shared sources: the rows every root feeds beside its own; everything that sizes, gathers or checks walks the roots */
    const SourceFans fans = S.source.empty() ? SourceFans() : sources_fans(S.source);
    std::vector<size_t> first((size_t)N), count((size_t)N);
    stream_need(S, length, first.data(), count.data());
    for (int i = 0; i < N; i++)
        if (count[(size_t)i] && !in_bytes[i]) return fail(ctx, GDG_ERR_INVALID, "input %d: the slice needs %zu frames from %zu on", i, count[(size_t)i], first[(size_t)i]);
    int rc = check_meter_ports(ctx, opt, "");
    if (rc != GDG_OK) return rc;
    enter(ctx);
    if ((rc = loudness_slice_begin(ctx, NR, pos, length, opt->target_rate)) != GDG_OK) return rc;      /* never a shard's: its calls refuse the switch */
    const int W = ctx->window;
    const size_t ws = (size_t)W * B;
    /* a shard's slice: the rows that leave the device encoded and as float64 are this slice's (which metronome buffers it passes), the
     * room for them is the job's (whether the shard runs the metronome): no slice makes a buffer grow */
    const int enc_rows = !sharded ? NR : N + (slice->metronome_bytes ? 1 : 0), f64_rows = !sharded ? 0 : 2 + (slice->metronome ? 1 : 0);
    const int enc_room = !sharded ? NR : N + (S.run_metro ? 1 : 0), f64_room = !sharded ? 0 : 2 + (S.run_metro ? 1 : 0);
    /* a half also holds, behind its rows, a window's section of every kind of the render report the call collects (report_sections.h) */
    const ReportLive live = report_live(ctx);
    const gdg_spectrum_bands bands = live.on(REPORT_BANDS) ? spectrum_bands(ctx->spec_live_edges.data(), (int)ctx->spec_live_edges.size(), opt->target_rate) : gdg_spectrum_bands();
    /* a shard that does not run the metronome measures nothing against that port */
    const std::vector<gdg_align_pairs> pairs = live.on(REPORT_ALIGN) ? align_map_pieces(ctx->align_live_ref, ctx->align_live_lag, (sharded && !S.run_metro) ? N : -1) : std::vector<gdg_align_pairs>();
    const size_t enc_bytes = ((deliver_ratio_window_bytes((size_t)W, R, RL, RM, (size_t)out_width, (size_t)enc_room) + 15) & ~(size_t)15) + (size_t)f64_room * ws * sizeof(double)
                           + report_room(live, (size_t)(sharded ? N + 1 : NR), (size_t)W) + lists_room(list_shape, (size_t)W);
    const size_t half = std::max(enc_bytes, (size_t)8 << 20);
    const UploadLayout L = upload_layout(S, N, ws);
    rc = ensure_batch_pipe(ctx, half, L.up_half);
    if (rc != GDG_OK) return rc;
    static int trace = -1;
    if (trace < 0) { const char *e = getenv("GDG_BATCH_TRACE"); trace = e ? atoi(e) : 0; }
    const double t_begin = now_ms();
    begun = true;
    auto body = [&]() -> int {
        int r;
        double *d_inputs = nullptr, *d_win = nullptr, *d_carry = nullptr;
        unsigned char *d_enc = nullptr, *d_up = nullptr, *d_src = nullptr;
        if ((r = batch_buffer(ctx, BATCH_INPUTS, (size_t)N * length * sizeof(double), (void **)&d_inputs)) != GDG_OK) return r;
        /* one window of the N + 3 outputs, rows in the output files' order (out_0 .. out_{N-1}, master left, master right, metronome,
         * controller.go:3123-3219), and behind them the rows of the blends in force; the inputs are read where they lie */
        if ((r = batch_buffer(ctx, BATCH_WINDOW, (size_t)NR * ws * sizeof(double), (void **)&d_win)) != GDG_OK) return r;
        if ((r = batch_buffer(ctx, BATCH_ENCODED, 2 * enc_bytes, (void **)&d_enc)) != GDG_OK) return r;
        if ((r = batch_carry_buffer(ctx, &d_carry)) != GDG_OK) return r;
        if ((r = batch_buffer(ctx, BATCH_UPLOAD, 2 * L.up_half, (void **)&d_up)) != GDG_OK) return r;
        if (L.src_half && (r = batch_buffer(ctx, BATCH_SOURCE, 2 * L.src_half, (void **)&d_src)) != GDG_OK) return r;
        /* the zero padding (controller.go:3018-3045): what no step of this slice will write */
        for (int i = 0; i < N; i++) {
            const size_t n_out = S.n_out[(size_t)i];
            const size_t covered = n_out <= pos ? 0 : std::min(n_out - pos, length);
            if (covered < length)
                HIP_TRY(ctx, hipMemsetAsync(d_inputs + (size_t)i * length + covered, 0, (length - covered) * sizeof(double), ctx->stream));
        }
        SliceStage stage_state = { ctx, S, in_bytes, L, fans, first, count, length, pos, d_inputs, d_carry, d_up, d_src, {}, { 0, 0 } };
        stage_state.run = S.brought;
        const BatchStage stage = std::ref(stage_state);
        BatchLoop loop{ N, enc_rows, f64_rows, out_width, W, length, ws, enc_bytes, d_inputs, d_win, d_enc, opt, out_bytes, slice, S.run_metro, L.any, trace, t_begin,
                        S.length / B, pos / B, live, gdg_dither_applies(ctx->dither_mode, opt->out_format), (uint64_t)pos, live.on(REPORT_BANDS) ? &bands : nullptr,
                        live.on(REPORT_ALIGN) ? &pairs : nullptr, nullptr, 0, {}, nullptr, nullptr, {} };
        if ((r = slice_settings(ctx, lists, n_blends, R, RL, RM, pos, blocks, loop)) != GDG_OK) return r;
        return batch_block_loop(ctx, loop, stage);
    };
    rc = body();
    hipStreamSynchronize(ctx->batch_up_stream);
    hipStreamSynchronize(ctx->batch_stream);
    hipStreamSynchronize(ctx->stream);
    /* the device buffers stay with the context for the next slice or job (gdg_batch_release) */
    brought.resize((size_t)N);
    for (int i = 0; i < N; i++) brought[(size_t)i] = first[(size_t)i] + count[(size_t)i];
    for (int i = 0; i < N; i++) if (is_reader(S, i)) brought[(size_t)i] = brought[(size_t)S.source[(size_t)i]];
    return loudness_slice_end(ctx, report_end(ctx, rc));
}

/* one slice of the context's open job; `slice`: of a job opened as a shard (the slice's partial master and metronome buffers) */
static int stream_step(gdg_ctx *ctx, int blocks, const void *const *in_bytes, void *const *out_bytes, const gdg_batch_shard_out *slice, bool as_shard) {
    if (!ctx) return GDG_ERR_INVALID;
    int rc = stream_check_blocks(ctx, blocks);
    if (rc != GDG_OK) return rc;
    auto &S = ctx->bstream;
    if (as_shard != S.shard)
        return fail(ctx, GDG_ERR_INVALID, as_shard ? "gdg_batch_stream_step_shard: the open job is not a shard's (gdg_batch_stream_open): gdg_batch_stream_step runs its slices"
                                                   : "gdg_batch_stream_step: the open job is a shard's (gdg_batch_stream_open_shard): gdg_batch_stream_step_shard runs its slices");
    if (!in_bytes || !out_bytes) return fail(ctx, GDG_ERR_INVALID, "a slice needs its input and output buffer lists");
    if (as_shard && (!slice || !slice->master_left || !slice->master_right)) return fail(ctx, GDG_ERR_INVALID, "a shard needs buffers for its partial master mix");
    if (as_shard && !S.run_metro && (slice->metronome_bytes || slice->metronome))
        return fail(ctx, GDG_ERR_INVALID, "this shard's job was opened without the metronome (run_metronome = 0): a slice cannot ask for its track");
    std::vector<size_t> brought;
    bool begun = false;
    rc = run_slice(ctx, S, blocks, in_bytes, out_bytes, as_shard ? slice : nullptr, brought, begun);
    if (rc != GDG_OK) { if (begun) S.open = false; return rc; }                 /* a slice that failed half-way: the job cannot go on */
    S.brought = brought;
    S.pos += (size_t)blocks * GDG_BLOCK_SIZE;
    return GDG_OK;
}

int gdg_batch_stream_step(gdg_ctx *ctx, int blocks, const void *const *in_bytes, void *const *out_bytes) {
    return stream_step(ctx, blocks, in_bytes, out_bytes, nullptr, false);
}

int gdg_batch_stream_step_shard(gdg_ctx *ctx, int blocks, const void *const *in_bytes, void *const *out_bytes, const gdg_batch_shard_out *slice) {
    if (ctx && delivery_on(ctx)) return DELIVERY_REFUSED(ctx, "gdg_batch_stream_step_shard");
    if (ctx && ctx->out_rec_on) return OUT_RECORDS_REFUSED(ctx, "gdg_batch_stream_step_shard");
    if (const int rl = loudness_refused(ctx, "gdg_batch_stream_step_shard", "a sharded job cannot collect them yet")) return rl;
    if (const int rc = lists_refused(ctx, "gdg_batch_stream_step_shard")) return rc;
    return stream_step(ctx, blocks, in_bytes, out_bytes, slice, true);
}

/* The one-call run (controller.processFiles in one call) is the single slice [0, job) of a job that is opened and closed inside the call:
 * a job of its own, never the context's, which stays closed throughout. */
static int batch_run_impl(gdg_ctx *ctx, const gdg_batch_input *inputs, int n_inputs, const gdg_batch_options *opt, void *const *out_bytes,
                          const gdg_batch_shard_out *shard) {
    if (!ctx || !inputs || !opt || !out_bytes) return GDG_ERR_INVALID;
    if (ctx->bstream.open) return fail(ctx, GDG_ERR_INVALID, "a streamed batch run is open on this context: gdg_batch_stream_close it first");
    /* One shard of a job split over several contexts: the master mix is the sum over ALL channels, then the aux input,
     * then the encoder's clip (spatializer.go:300-310, controller.go:3123-3219) -- so a shard hands out its PARTIAL sums as float64
     * and gdg_batch_finish_master adds the shards' partials in shard order, then aux, then encodes.  The metronome runs on the shard
     * that is given somewhere to put it. */
    if (shard && (!shard->master_left || !shard->master_right)) return fail(ctx, GDG_ERR_INVALID, "a shard needs buffers for its partial master mix");
    gdg_ctx::BatchStreamState job;
    int rc = stream_job(ctx, inputs, n_inputs, opt, shard != nullptr, shard ? shard->job_samples : 0, shard && (shard->metronome_bytes || shard->metronome), job,
                        /*meters_at_open=*/false);
    if (rc != GDG_OK) return rc;
    for (int i = 0; i < n_inputs; i++)                                           /* a one-call run holds its inputs' rows whole: gdg_batch_length's bound */
        if (job.inputs[(size_t)i].bytes && job.inputs[(size_t)i].samples_per_channel > 0x7fffffff) return fail(ctx, GDG_ERR_INVALID, "input %d is too long", i);
    if (job.length == 0) {                                                       /* every output has 0 samples */
        ctx->batch_up_bytes = ctx->batch_resampled = 0;
        report_begin(ctx, shard ? n_inputs + 1 : n_inputs + 3 + ctx->blend.count(), 0, true, shard ? 0 : ctx->blend.count());
        for (int k = 0; k < LIST_KINDS && !shard; k++) list_begin(ctx, k, 0, n_inputs + 3 + ctx->blend.count());
        return report_end(ctx, GDG_OK);
    }
    if ((rc = check_meter_ports(ctx, opt, SHARD_PORTS)) != GDG_OK) return rc;
    if (job.length > 0x7fffffff) return fail(ctx, GDG_ERR_INVALID, "files of %zu samples are too long", job.length);
    std::vector<const void *> in_bytes((size_t)n_inputs);
    for (int i = 0; i < n_inputs; i++) in_bytes[(size_t)i] = inputs[i].bytes;       /* a reader's is never read */
    std::vector<size_t> brought;
    bool begun = false;
    return run_slice(ctx, job, (int)(job.length / GDG_BLOCK_SIZE), in_bytes.data(), out_bytes, shard, brought, begun);
}

int gdg_batch_run(gdg_ctx *ctx, const gdg_batch_input *inputs, int n_inputs, const gdg_batch_options *opt, void *const *out_bytes) {
    return batch_run_impl(ctx, inputs, n_inputs, opt, out_bytes, nullptr);
}

int gdg_batch_run_shard(gdg_ctx *ctx, const gdg_batch_input *inputs, int n_inputs, const gdg_batch_options *opt, void *const *out_bytes,
                        const gdg_batch_shard_out *shard) {
    if (!shard) return GDG_ERR_INVALID;
    if (ctx && delivery_on(ctx)) return DELIVERY_REFUSED(ctx, "gdg_batch_run_shard");
    if (ctx && ctx->out_rec_on) return OUT_RECORDS_REFUSED(ctx, "gdg_batch_run_shard");
    if (const int rl = loudness_refused(ctx, "gdg_batch_run_shard", "a sharded job cannot collect them yet")) return rl;
    if (ctx && ctx->blend.count()) return BLENDS_REFUSED(ctx, "gdg_batch_run_shard");
    if (const int rc = lists_refused(ctx, "gdg_batch_run_shard")) return rc;
    /* a shard's master mix is a PARTIAL sum: the aux input joins the master once, in gdg_batch_finish_master (its `aux` = the float64
     * metronome track of the shard that ran it).  A set flag here would be silently dropped -- refuse it instead. */
    if (ctx && opt && opt->metronome_to_master)
        return fail(ctx, GDG_ERR_INVALID, "gdg_batch_run_shard: metronome_to_master must be 0 -- a shard's master mix is a partial sum; pass the metronome's float64 "
                    "track (gdg_batch_shard_out.metronome of the shard that runs it) as `aux` to gdg_batch_finish_master");
    return batch_run_impl(ctx, inputs, n_inputs, opt, out_bytes, shard);
}

/* what both forms of the master mix refuse, in this order */
static int finish_master_check(gdg_ctx *ctx, int out_format, const double *const *left, const double *const *right, int n_shards, uint32_t sample_rate,
                               int run_meters) {
    if (!ctx || !left || !right || n_shards <= 0) return GDG_ERR_INVALID;
    if (!gdg_wave_bytes_per_sample(out_format)) return fail(ctx, GDG_ERR_UNSUPPORTED, "unknown sample format %d", out_format);
    for (int g = 0; g < n_shards; g++) if (!left[g] || !right[g]) return fail(ctx, GDG_ERR_INVALID, "shard %d has no partial master mix", g);
    if (run_meters && (ctx->n_meter < 2 || sample_rate == 0)) return fail(ctx, GDG_ERR_INVALID, "master meters: the context's last two ports, at a positive rate");
    return GDG_OK;
}

/* what the master mix keeps on the context: its events, its two pairs of pinned halves, and on the device two slab halves (+ the two rows of
 * sums the meters read, sums_bytes) and two halves of encoded rows */
static int finish_master_room(gdg_ctx *ctx, size_t up_bytes, size_t down_bytes, size_t sums_bytes) {
    if (!ctx->fin_up[0])
        for (int h = 0; h < 2; h++) {
            HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->fin_up[h], hipEventDisableTiming));
            HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->fin_down[h], hipEventDisableTiming));
        }
    HIP_TRY(ctx, ctx->h_fin_up.grow(ctx, up_bytes));
    HIP_TRY(ctx, ctx->h_fin_down.grow(ctx, down_bytes));
    const int rc = ensure_io(ctx, 1, 2 * up_bytes + sums_bytes);
    return rc != GDG_OK ? rc : ensure_io(ctx, 0, 2 * down_bytes);
}

/* the samples [at, at + n) of the G partial pairs and aux (null: none) into a pinned half: [left_0 .. left_{G-1} | right_0 .. right_{G-1} | aux],
 * stride samples apart, the samples behind each row zeros */
static void finish_master_gather(gdg_ctx *ctx, unsigned char *half, const double *const *left, const double *const *right, size_t G, const double *aux, size_t at,
                                 size_t n, size_t stride) {
    std::vector<BatchPiece> pieces;
    for (size_t r = 0; r < 2 * G + (aux ? 1 : 0); r++) {
        const double *src = (r < G ? left[r] : r < 2 * G ? right[r - G] : aux) + at;
        unsigned char *row = half + r * stride * sizeof(double);
        for (size_t q = 0; q < n * sizeof(double); q += (size_t)1 << 18)      /* pieces of <= 256 KiB: every worker gets some */
            pieces.push_back({ row + q, reinterpret_cast<const unsigned char *>(src) + q, std::min(n * sizeof(double) - q, (size_t)1 << 18) });
        memset(row + n * sizeof(double), 0, (stride - n) * sizeof(double));
    }
    move_pieces(ctx, pieces);
}

/* The master mix of a sharded job, or of one slice of it: master =((p_0 + p_1) + ... + p_{G-1}) + aux per side, then the encoder (its clip
 * included) -- all on this context's device, per piece ONE upload, ONE kernel and ONE download.  The copy workers gather the G partial
 * pairs and aux into a pinned slab half ([2 G + 1][stride] float64) while the piece before is on the bus; finish_master_kernel (io.hip)
 * adds and encodes; the encoded piece comes down into a pinned half and is scattered into the caller's buffers while the next piece
 * computes.  Pieces are whole blocks but for the last, which has whatever is left (n >= 1): its rows lie stride = n rounded up to 4 samples
 * apart, the gather writes the 0 .. 3 samples behind each row as zeros, the kernel runs over stride / 4 groups, and what it makes of the
 * pad stays on the device -- the meters, the report and the download take n samples. */
static int finish_master(gdg_ctx *ctx, int out_format, const double *const *left, const double *const *right, int n_shards, const double *aux,
                         size_t samples, uint32_t sample_rate, int run_meters, void *left_bytes, void *right_bytes, uint64_t dither_first) {
    const size_t width = (size_t)gdg_wave_bytes_per_sample(out_format), B = GDG_BLOCK_SIZE;
    report_begin(ctx, 2, (samples + B - 1) / B, /*align=*/false);                /* the master's two sides: no alignment records (include/gdg.h) */
    if (!ctx->spec_live_edges.empty() && sample_rate == 0)                       /* like every refusal from here on: the call before's report and spectrum are gone */
        return report_end(ctx, fail(ctx, GDG_ERR_INVALID, "master mix: the band spectrum needs a positive sample rate"));
    if (samples == 0) return report_end(ctx, GDG_OK);
    const ReportLive live = report_live(ctx);                                    /* never the alignment records: report_begin above */
    const bool dither = gdg_dither_applies(ctx->dither_mode, out_format), spectrum = live.on(REPORT_BANDS);
    /* the trim in force on the context that finishes: its two master gains, as kernel arguments */
    const bool trim = !ctx->trim_gain.empty();
    const double trim_left = trim ? ctx->trim_gain[(size_t)ctx->nch + GDG_TRIM_MASTER_LEFT] : 1.0, trim_right = trim ? ctx->trim_gain[(size_t)ctx->nch + GDG_TRIM_MASTER_RIGHT] : 1.0;
    enter(ctx);
    const gdg_spectrum_bands bands = spectrum ? spectrum_bands(ctx->spec_live_edges.data(), (int)ctx->spec_live_edges.size(), sample_rate) : gdg_spectrum_bands();
    SpectrumTables spec = { &bands, nullptr, nullptr, nullptr };
    if (spectrum) { const int rs = spectrum_tables(ctx, &spec.win, &spec.tw, &spec.tw2); if (rs != GDG_OK) return report_end(ctx, rs); }
    const size_t G = (size_t)n_shards, rows = 2 * G + (aux ? 1 : 0);
    /* a piece: whole blocks, a slab half of at most 8 MiB (one block at least) -- bounded whatever the sample count and the shard count */
    const size_t piece = B * std::min((size_t)128, std::max((size_t)1, ((size_t)8 << 20) / ((2 * G + 1) * B * sizeof(double))));
    /* the render report: a piece's section of every live kind, [2][piece / 8192], comes down behind its encoded rows, packed */
    const ReportSections sec = report_sections(live, 2, piece / B, 2 * piece * width, false);
    const size_t up_bytes = (2 * G + 1) * piece * sizeof(double), down_bytes = sec.end;
    const std::vector<size_t> both_sides = { 0, 1 };
    int rc = finish_master_room(ctx, up_bytes, down_bytes, 2 * piece * sizeof(double));
    if (rc != GDG_OK) return rc;
    unsigned char *d_slab = static_cast<unsigned char *>(ctx->d_io[1]), *d_enc = static_cast<unsigned char *>(ctx->d_io[0]);
    double *d_sums = (run_meters || live.any()) ? reinterpret_cast<double *>(d_slab + 2 * up_bytes) : nullptr;
    const size_t n_pieces = (samples + piece - 1) / piece;
    auto span = [&](size_t k) { return std::min(piece, samples - k * piece); };
    auto stride_of = [](size_t n) { return (n + 3) & ~(size_t)3; };                /* <= piece: a piece is whole blocks */
    auto body = [&]() -> int {
        /* piece k's rows into its pinned half: [left_0 .. left_{G-1} | right_0 .. right_{G-1} | aux], stride samples apart */
        auto gather = [&](size_t k) -> int {
            const int h = (int)(k & 1);
            const size_t n = span(k);
            if (k >= 2) HIP_TRY(ctx, hipEventSynchronize(ctx->fin_up[h]));     /* piece k - 2 has left this half */
            finish_master_gather(ctx, ctx->h_fin_up[h], left, right, G, aux, k * piece, n, stride_of(n));
            return GDG_OK;
        };
        auto enqueue = [&](size_t k) -> int {
            const int h = (int)(k & 1);
            const size_t n = span(k), stride = stride_of(n), nb = (n + B - 1) / B;
            unsigned char *slab = d_slab + (size_t)h * up_bytes, *enc = d_enc + (size_t)h * down_bytes;
            HIP_TRY(ctx, hipMemcpyAsync(slab, ctx->h_fin_up[h], rows * stride * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(ctx, hipEventRecord(ctx->fin_up[h], ctx->stream));
            {
                ProfScope ps(ctx, GDG_K_WAVE);
                /* the sums stay as they are; the encoder reads them times the gains.  The piece's first sample: dither_first + k * piece */
                const gdg_encode_mode m = { trim, dither, nullptr, { trim_left, trim_right }, { ctx->dither_seed, dither_first + k * piece, 0, 0 } };
                HIP_TRY(ctx, gdg_launch_finish_master(out_format, reinterpret_cast<const double *>(slab), stride, n_shards, aux != nullptr, stride, enc, enc + piece * width,
                                                      d_sums, piece, m, ctx->stream));
            }
            if (run_meters)
                for (size_t o = 0; o < n; o += B)                                /* block by block, like the loop that fed the other ports */
                    if ((rc = meter_rows(ctx, d_sums + o, piece, ctx->n_meter - 2, 2, (int)std::min(B, n - o), sample_rate)) != GDG_OK) return rc;
            /* the records of the sums, after the aux and before the encoder's clamp: a short last block is zero-padded by the spectrum's kernel
             * and just shorter for the true peak's; then every live kind's [2][nb] elements of this piece on their way down */
            const RowGroup sums = { d_sums, piece, 2u, 0 };
            if ((rc = port_records(ctx, { REPORT_STATS, REPORT_BANDS, REPORT_TRUE_PEAK }, &sums, 1, n, nb, live, sec, enc, spec)) != GDG_OK) return rc;
            for (int j = 0; j < REPORT_KINDS; j++)
                if (live.on(j)) HIP_TRY(ctx, hipMemcpyAsync(ctx->h_fin_down[h] + sec.at[j], enc + sec.at[j], 2 * nb * live.elem[j], hipMemcpyDeviceToHost, ctx->stream));
            /* the download of piece k - 2 into this pinned half has been scattered: scatter(k - 2) ran before enqueue(k) */
            if (left_bytes) HIP_TRY(ctx, hipMemcpyAsync(ctx->h_fin_down[h], enc, n * width, hipMemcpyDeviceToHost, ctx->stream));
            if (right_bytes) HIP_TRY(ctx, hipMemcpyAsync(ctx->h_fin_down[h] + piece * width, enc + piece * width, n * width, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipEventRecord(ctx->fin_down[h], ctx->stream));
            return GDG_OK;
        };
        auto scatter = [&](size_t k) -> int {
            const int h = (int)(k & 1);
            const size_t bytes = span(k) * width, at = k * piece * width;
            HIP_TRY(ctx, hipEventSynchronize(ctx->fin_down[h]));
            std::vector<BatchPiece> pieces;
            for (int side = 0; side < 2; side++) {
                unsigned char *dst = static_cast<unsigned char *>(side ? right_bytes : left_bytes);
                if (!dst) continue;
                const unsigned char *src = ctx->h_fin_down[h] + (size_t)side * piece * width;
                for (size_t q = 0; q < bytes; q += (size_t)1 << 18) pieces.push_back({ dst + at + q, src + q, std::min(bytes - q, (size_t)1 << 18) });
            }
            move_pieces(ctx, pieces);
            for (int j = 0; j < REPORT_KINDS; j++)                           /* the piece's sections: two rows of its blocks, filed under them */
                if (live.on(j)) report_file(ctx, j, ctx->h_fin_down[h] + sec.at[j], both_sides, (span(k) + B - 1) / B, k * (piece / B));
            return GDG_OK;
        };
        int r;
        if ((r = gather(0)) != GDG_OK || (r = enqueue(0)) != GDG_OK) return r;
        for (size_t k = 0; k < n_pieces; k++) {
            if (k + 1 < n_pieces && (r = gather(k + 1)) != GDG_OK) return r;    /* while piece k is on the bus */
            if (k >= 1 && (r = scatter(k - 1)) != GDG_OK) return r;             /* frees the pinned half piece k + 1 comes down into */
            if (k + 1 < n_pieces && (r = enqueue(k + 1)) != GDG_OK) return r;
        }
        return scatter(n_pieces - 1);
    };
    rc = body();
    hipStreamSynchronize(ctx->stream);                                           /* the caller's rows are never read after the call, whatever happened */
    return report_end(ctx, rc);
}

/* the master mix of a whole job: any sample count */
int gdg_batch_finish_master(gdg_ctx *ctx, int out_format, const double *const *left, const double *const *right, int n_shards, const double *aux,
                            size_t samples, uint32_t sample_rate, int run_meters, void *left_bytes, void *right_bytes) {
    if (ctx && delivery_on(ctx)) return DELIVERY_REFUSED(ctx, "gdg_batch_finish_master");
    if (ctx && ctx->out_rec_on) return OUT_RECORDS_REFUSED(ctx, "gdg_batch_finish_master");
    if (const int rl = loudness_refused(ctx, "gdg_batch_finish_master", "a master mix has no hop records yet")) return rl;
    const int rc = finish_master_check(ctx, out_format, left, right, n_shards, sample_rate, run_meters);
    if (rc != GDG_OK) return rc;
    return finish_master(ctx, out_format, left, right, n_shards, aux, samples, sample_rate, run_meters, left_bytes, right_bytes, 0);      /* the cursor stays */
}

/* ... and of one slice of a streamed sharded job, where it runs once per slice on the job's critical path: whole blocks, as the slices are */
int gdg_batch_finish_master_slice(gdg_ctx *ctx, int out_format, const double *const *left, const double *const *right, int n_shards, const double *aux,
                                  size_t samples, uint32_t sample_rate, int run_meters, void *left_bytes, void *right_bytes) {
    if (ctx && delivery_on(ctx)) return DELIVERY_REFUSED(ctx, "gdg_batch_finish_master_slice");
    if (ctx && ctx->out_rec_on) return OUT_RECORDS_REFUSED(ctx, "gdg_batch_finish_master_slice");
    if (const int rl = loudness_refused(ctx, "gdg_batch_finish_master_slice", "a master mix has no hop records yet")) return rl;
    const int rc = finish_master_check(ctx, out_format, left, right, n_shards, sample_rate, run_meters);
    if (rc != GDG_OK) return rc;
    if (samples % GDG_BLOCK_SIZE) return fail(ctx, GDG_ERR_INVALID, "a slice of %zu samples: whole blocks of %d", samples, GDG_BLOCK_SIZE);
    /* the slice starts at the master cursor (gdg_batch_dither_seek) and a finished slice moves it on, dither on or off */
    uint64_t next = ctx->dither_cursor + samples;
    if (ctx->dither_mode && !gdg_dither_advance(ctx->dither_cursor, samples, &next))
        return fail(ctx, GDG_ERR_INVALID, "a slice of %zu samples from sample index %llu on passes 2^64", samples, (unsigned long long)ctx->dither_cursor);
    const int r = finish_master(ctx, out_format, left, right, n_shards, aux, samples, sample_rate, run_meters, left_bytes, right_bytes, ctx->dither_cursor);
    if (r == GDG_OK) ctx->dither_cursor = next;
    return r;
}
