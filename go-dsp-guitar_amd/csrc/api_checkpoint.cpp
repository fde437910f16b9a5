/*
 * api_checkpoint.cpp -- a streamed batch run written into one blob between two slices and continued from it in another context
 * (gdg_batch_stream_checkpoint / _resume, gdg_state_verify; include/gdg.h documents the container, its rules and the digest).
 * Part of the host side of libgdg.so (the C-ABI of include/gdg.h on top of the HIP kernels; see ctx.h for the map).
 *
 * The container wraps the channel-state blob of api_state.cpp (version 1, unchanged) and adds what a streamed job carries beside it: the
 * job's position, the source frames the resampler looks back at, the meter records, the tuner rings and the metronome's counters.  The
 * device side is the state blob's: the rings, records and frames are more pieces {src, dst, bytes} of the SAME launch of state.hip's copy
 * kernel; the payload never passes through the host except in the one copy to or from the caller's buffer.  The digest is taken on the
 * device, over the staged copy: after the gather of a checkpoint, before anything is checked or written in a resume.
 */
#include "ctx.h"

#define GDG_CKPT_MAGIC "GDGCKPT"           /* + the terminating zero: 8 bytes */
#define GDG_CKPT_VERSION 1u
#define GDG_BLOCK_SIZE 8192                /* controller/controller.go:36 */

enum { SEC_JOB, SEC_STATE, SEC_METERS, SEC_TUNER, SEC_METRONOME, SEC_CARRY, SEC_COUNT };
static const char *const section_names[SEC_COUNT] = { "job", "channel state", "meters", "tuner", "metronome", "resampler carry" };

/* little-endian, natural alignment, no padding the compiler adds (static_asserts below) */
struct CkptHeader {
    char magic[8];
    uint32_t version, payload_off;         /* the payload is [payload_off, total_bytes): a whole number of 16-byte granules */
    uint64_t total_bytes;
    uint64_t reserved;
    uint64_t digest[2];                    /* of the payload (include/gdg.h) */
};
struct CkptSection { uint64_t off, bytes; };                 /* from the container's start; bytes == 0: not present */
struct CkptDir { CkptSection s[SEC_COUNT]; };                /* the payload's first bytes */
struct CkptJob {
    uint32_t n_inputs, shard, run_metronome, target_rate;
    int32_t out_format, metronome_to_master, run_meters, tuner_enqueue;
    uint64_t length, pos;                                    /* samples of every output (a shard: the job's), samples done */
};
struct CkptInput {                                           /* n_inputs of them behind the job */
    uint64_t samples_per_channel, brought, n_out;
    int32_t format;
    uint32_t sample_rate, channels, channel, has_samples, carry_valid;     /* carry_valid: frames of its carry that hold source frames */
};
struct CkptMeterHead { uint32_t ports, record_bytes; uint64_t reserved; };      /* then `ports` records {current, peak, counter, enabled} */
struct CkptTunerHead { uint32_t rate, wp, ring_len, channels; };                /* then the rings, OLDEST SAMPLE FIRST (wp: the source's, informative) */
struct CkptMetronome { uint32_t sample_counter, tick_counter; uint64_t reserved; };
static_assert(sizeof(CkptHeader) == 48, "container header layout");
static_assert(sizeof(CkptDir) == 96, "container directory layout");
static_assert(sizeof(CkptJob) == 48 && sizeof(CkptInput) == 48, "job section layout");
static_assert(sizeof(CkptMeterHead) == 16 && sizeof(CkptTunerHead) == 16 && sizeof(CkptMetronome) == 16, "section head layout");
static_assert(sizeof(gdg_meter_rec) == 32, "meter record layout");

/* ---- the digest -------------------------------------------------------------------------------------------------------------------- */
static inline uint64_t fmix64(uint64_t x) {
    x ^= x >> 33; x *= GDG_DIGEST_M0;
    x ^= x >> 33; x *= GDG_DIGEST_M1;
    x ^= x >> 33;
    return x;
}

/* of the container on the device whose header says `total` bytes: state.hip's partial sums, added up and finished here */
static int payload_digest(gdg_ctx *ctx, const unsigned char *d_blob, size_t total, uint64_t out[2]) {
    const unsigned long long granules = (total - sizeof(CkptHeader)) / 16;
    uint64_t s0 = 0, s1 = 0;
    if (granules) {
        const unsigned long long per_group = 256 * 4;
        const int groups = (int)std::min<unsigned long long>(GDG_DIGEST_GROUPS, (granules + per_group - 1) / per_group);
        unsigned long long *d_part = nullptr;
        HIP_TRY(ctx, ctx->arena.alloc((void **)&d_part, (size_t)groups * 16));
        std::vector<unsigned long long> part((size_t)groups * 2, 0);
        hipError_t e = gdg_launch_state_digest(d_blob + sizeof(CkptHeader), granules, d_part, groups, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(part.data(), d_part, part.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream);
        hipError_t w = hipStreamSynchronize(ctx->stream);
        ctx->arena.release(d_part);
        if (e != hipSuccess || w != hipSuccess) return fail(ctx, GDG_ERR_HIP, "checkpoint digest: %s", hipGetErrorString(e != hipSuccess ? e : w));
        for (int g = 0; g < groups; g++) { s0 += part[2 * (size_t)g]; s1 ^= part[2 * (size_t)g + 1]; }
    }
    out[0] = fmix64(s0 + GDG_DIGEST_K + granules);
    out[1] = fmix64(s1 ^ out[0]);
    return GDG_OK;
}

/* ---- layout -------------------------------------------------------------------------------------------------------------------------- */
struct CkptPlan { CkptDir dir; size_t total; };

static int checkpoint_plan(gdg_ctx *ctx, CkptPlan &P) {
    size_t state_bytes = 0;
    const int rc = gdg_state_size(ctx, nullptr, 0, &state_bytes);
    if (rc != GDG_OK) return rc;
    const size_t N = (size_t)ctx->nch;
    memset(&P.dir, 0, sizeof(P.dir));
    size_t off = sizeof(CkptHeader) + sizeof(CkptDir);
    auto put = [&](int sec, size_t bytes) { P.dir.s[sec] = CkptSection{ bytes ? off : 0, bytes }; off += round16(bytes); };
    put(SEC_JOB, sizeof(CkptJob) + N * sizeof(CkptInput));
    put(SEC_METRONOME, sizeof(CkptMetronome));
    put(SEC_CARRY, N * GDG_STREAM_CARRY * sizeof(double));
    put(SEC_METERS, sizeof(CkptMeterHead) + (size_t)ctx->n_meter * sizeof(gdg_meter_rec));
    put(SEC_TUNER, ctx->d_tuner_ring ? sizeof(CkptTunerHead) + N * GDG_TUNER_RING * sizeof(double) : 0);
    put(SEC_STATE, state_bytes);
    P.total = off;
    return GDG_OK;
}

/* version 1 records positions and resampler carries per input; a reader has neither of its own */
#define SHARED_SOURCES_REFUSED(ctx, what) \
    fail(ctx, GDG_ERR_UNSUPPORTED, "%s: a job with shared sources (gdg_batch_set_sources: a channel reads another's input) cannot be checkpointed yet", what)
/* ... and nothing of the blend history (gdg_batch_set_blends_delayed, gdg_batch_set_blends_filtered): the chain rows' last samples, which a
 * delayed or filtered term reads */
#define BLEND_HISTORY_REFUSED(ctx, what) \
    fail(ctx, GDG_ERR_UNSUPPORTED, "%s: a blend term reaches up to %d samples back (gdg_batch_set_blends_delayed, gdg_batch_set_blends_filtered); the blend history is not in the version-1 container", what, \
         (ctx)->blend.max_reach())
/* ... nor of the delivery history (gdg_batch_set_delivery): the window rows' last 154 samples, which the next step's first outputs read */
static int delivery_history_refused(gdg_ctx *ctx, const char *what) {
    if (gdg_deliver_ratio_on(ctx->deliver_up, ctx->deliver_down))
        return fail(ctx, GDG_ERR_UNSUPPORTED, "%s: the delivery factor %d with the delivery ratio %d/%d is in force on this context (gdg_batch_set_out_ratio); the delivery histories are not in the version-1 container",
                    what, ctx->deliver, ctx->deliver_up, ctx->deliver_down);
    return fail(ctx, GDG_ERR_UNSUPPORTED, "%s: the delivery factor %d is in force on this context (gdg_batch_set_delivery); the delivery history is not in the version-1 container", what, ctx->deliver);
}
#define DELIVERY_HISTORY_REFUSED(ctx, what) delivery_history_refused(ctx, what)
/* ... nor of the delivered rows' records' (gdg_batch_out_records_enable): the 23 samples in front of the next step's first block */
#define OUT_RECORDS_HISTORY_REFUSED(ctx, what) \
    fail(ctx, GDG_ERR_UNSUPPORTED, "%s: the delivered rows' records are on on this context (gdg_batch_out_records_enable); their history is not in the version-1 container", what)
static bool input_has_samples(const gdg_batch_input &in) { return in.bytes && in.samples_per_channel; }
/* the frames of input i's carry that hold source frames: what the next step of the job will read from it (api_batch.cpp, stream_step) */
static uint32_t carry_valid(const gdg_ctx::BatchStreamState &S, size_t i) {
    const gdg_batch_input &in = S.inputs[i];
    if (!input_has_samples(in) || in.sample_rate == S.opt.target_rate) return 0;
    return (uint32_t)std::min(S.brought[i], (size_t)GDG_STREAM_CARRY);
}

int gdg_batch_stream_checkpoint_size(gdg_ctx *ctx, size_t *bytes) {
    if (!ctx || !bytes) return GDG_ERR_INVALID;
    if (batch_sources_shared(ctx)) return SHARED_SOURCES_REFUSED(ctx, "checkpoint");
    if (ctx->blend.max_reach() > 0) return BLEND_HISTORY_REFUSED(ctx, "checkpoint");
    if (delivery_on(ctx)) return DELIVERY_HISTORY_REFUSED(ctx, "checkpoint");
    if (ctx->out_rec_on) return OUT_RECORDS_HISTORY_REFUSED(ctx, "checkpoint");
    if (const int rl = loudness_refused(ctx, "checkpoint", "their state is not in the version-1 container")) return rl;
    if (!ctx->bstream.open) return fail(ctx, GDG_ERR_INVALID, "checkpoint: no streamed batch run is open on this context");
    CkptPlan P;
    const int rc = checkpoint_plan(ctx, P);
    if (rc == GDG_OK) *bytes = P.total;
    return rc;
}

int gdg_batch_stream_checkpoint(gdg_ctx *ctx, void *blob, size_t capacity, size_t *written) {
    if (!ctx || !blob) return GDG_ERR_INVALID;
    const auto &S = ctx->bstream;
    if (batch_sources_shared(ctx)) return SHARED_SOURCES_REFUSED(ctx, "checkpoint");
    if (ctx->blend.max_reach() > 0) return BLEND_HISTORY_REFUSED(ctx, "checkpoint");
    if (delivery_on(ctx)) return DELIVERY_HISTORY_REFUSED(ctx, "checkpoint");
    if (ctx->out_rec_on) return OUT_RECORDS_HISTORY_REFUSED(ctx, "checkpoint");
    if (const int rl = loudness_refused(ctx, "checkpoint", "their state is not in the version-1 container")) return rl;
    if (!S.open) return fail(ctx, GDG_ERR_INVALID, "checkpoint: no streamed batch run is open on this context");
    CkptPlan P;
    int rc = checkpoint_plan(ctx, P);
    if (rc != GDG_OK) return rc;
    if (written) *written = P.total;
    if (capacity < P.total)
        return fail(ctx, GDG_ERR_INVALID, "checkpoint: %zu bytes of capacity, the job takes %zu (gdg_batch_stream_checkpoint_size)", capacity, P.total);
    /* ordered after everything queued on the context; nothing it made ahead is dropped (a checkpoint changes no state) */
    enter(ctx, /*read_only=*/true);
    const size_t N = (size_t)ctx->nch;
    /* 1. what the host knows: header, directory, job, metronome -- one contiguous piece of the container -- and the two section heads */
    const size_t head_bytes = (size_t)P.dir.s[SEC_CARRY].off;
    std::vector<unsigned char> head(head_bytes, 0);
    CkptHeader h;
    memset(&h, 0, sizeof(h));
    memcpy(h.magic, GDG_CKPT_MAGIC, 8);
    h.version = GDG_CKPT_VERSION;
    h.payload_off = (uint32_t)sizeof(CkptHeader);
    h.total_bytes = P.total;
    memcpy(&head[sizeof(CkptHeader)], &P.dir, sizeof(P.dir));
    CkptJob j;
    memset(&j, 0, sizeof(j));
    j.n_inputs = (uint32_t)N;
    j.shard = S.shard; j.run_metronome = S.run_metro;
    j.target_rate = S.opt.target_rate; j.out_format = S.opt.out_format;
    j.metronome_to_master = S.opt.metronome_to_master != 0; j.run_meters = S.opt.run_meters != 0; j.tuner_enqueue = S.opt.tuner_enqueue != 0;
    j.length = S.length; j.pos = S.pos;
    memcpy(&head[P.dir.s[SEC_JOB].off], &j, sizeof(j));
    for (size_t i = 0; i < N; i++) {
        const gdg_batch_input &in = S.inputs[i];
        CkptInput r;
        memset(&r, 0, sizeof(r));
        r.has_samples = input_has_samples(in);
        if (r.has_samples) {
            r.samples_per_channel = in.samples_per_channel; r.format = in.format; r.sample_rate = in.sample_rate;
            r.channels = in.channels; r.channel = in.channel;
        }
        r.brought = S.brought[i]; r.n_out = S.n_out[i];
        r.carry_valid = carry_valid(S, i);
        memcpy(&head[P.dir.s[SEC_JOB].off + sizeof(j) + i * sizeof(r)], &r, sizeof(r));
    }
    CkptMetronome m = { ctx->met_sample_counter, ctx->met_tick_counter, 0 };
    memcpy(&head[P.dir.s[SEC_METRONOME].off], &m, sizeof(m));
    const CkptMeterHead mh = { (uint32_t)ctx->n_meter, (uint32_t)sizeof(gdg_meter_rec), 0 };
    const CkptTunerHead th = { ctx->tuner_sr, (uint32_t)ctx->tuner_wp, GDG_TUNER_RING, (uint32_t)N };

    unsigned char *stage = nullptr;
    HIP_TRY(ctx, ctx->arena.alloc((void **)&stage, P.total));
    auto body = [&]() -> int {
        memcpy(head.data(), &h, sizeof(h));
        HIP_TRY(ctx, hipMemcpyAsync(stage, head.data(), head.size(), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(stage + P.dir.s[SEC_METERS].off, &mh, sizeof(mh), hipMemcpyHostToDevice, ctx->stream));
        if (P.dir.s[SEC_TUNER].bytes) HIP_TRY(ctx, hipMemcpyAsync(stage + P.dir.s[SEC_TUNER].off, &th, sizeof(th), hipMemcpyHostToDevice, ctx->stream));
        /* 2. what the device holds, as more pieces of the state save's one launch */
        Pieces extra;
        const double *d_carry = ctx->batch_dev_cap[BATCH_CARRY] >= N * GDG_STREAM_CARRY * sizeof(double) ? static_cast<const double *>(ctx->batch_dev[BATCH_CARRY]) : nullptr;
        for (size_t i = 0; i < N; i++) {
            unsigned char *dst = stage + P.dir.s[SEC_CARRY].off + i * GDG_STREAM_CARRY * sizeof(double);
            const size_t valid = d_carry ? carry_valid(S, i) * sizeof(double) : 0;
            extra.add(d_carry ? d_carry + i * GDG_STREAM_CARRY : nullptr, dst, valid);
            extra.add(nullptr, dst + valid, GDG_STREAM_CARRY * sizeof(double) - valid);
        }
        extra.add(ctx->d_meter, stage + P.dir.s[SEC_METERS].off + sizeof(mh), (size_t)ctx->n_meter * sizeof(gdg_meter_rec));
        if (P.dir.s[SEC_TUNER].bytes) {
            const size_t wp = (size_t)ctx->tuner_wp, tail = GDG_TUNER_RING - wp;
            for (size_t c = 0; c < N; c++) {                     /* the oldest sample sits at the write position: two pieces around the ring's end */
                const double *ring = ctx->d_tuner_ring + c * GDG_TUNER_RING;
                double *dst = reinterpret_cast<double *>(stage + P.dir.s[SEC_TUNER].off + sizeof(th)) + c * GDG_TUNER_RING;
                extra.add(ring + wp, dst, tail * sizeof(double));
                extra.add(ring, dst + tail, wp * sizeof(double));
            }
        }
        int r = state_save_device_with(ctx, stage + P.dir.s[SEC_STATE].off, (size_t)P.dir.s[SEC_STATE].bytes, &extra);
        if (r != GDG_OK) return r;
        /* 3. the digest of what was just written, then the one copy to the caller */
        if ((r = payload_digest(ctx, stage, P.total, h.digest)) != GDG_OK) return r;
        HIP_TRY(ctx, hipMemcpy(blob, stage, P.total, hipMemcpyDeviceToHost));
        memcpy(blob, &h, sizeof(h));
        return GDG_OK;
    };
    rc = body();
    hipStreamSynchronize(ctx->stream);
    ctx->arena.release(stage);
    return rc;
}

/* ---- verify and resume --------------------------------------------------------------------------------------------------------------- */

/* The container's frame: magic, version, sizes.  `what`: the call's name for messages. */
static int read_header(gdg_ctx *ctx, const char *what, const void *blob, size_t bytes, CkptHeader &h) {
    if (bytes >= 8 && memcmp(blob, "GDGSTATE", 8) == 0)
        return fail(ctx, GDG_ERR_INVALID, "%s: a bare channel-state blob (GDGSTATE) carries no digest: only a checkpoint container (gdg_batch_stream_checkpoint) does", what);
    if (bytes < sizeof(CkptHeader) + sizeof(CkptDir)) return fail(ctx, GDG_ERR_INVALID, "%s: %zu bytes are no checkpoint (truncated)", what, bytes);
    memcpy(&h, blob, sizeof(h));
    if (memcmp(h.magic, GDG_CKPT_MAGIC, 8) != 0) return fail(ctx, GDG_ERR_INVALID, "%s: not a checkpoint (bad magic)", what);
    if (h.version != GDG_CKPT_VERSION)
        return fail(ctx, GDG_ERR_INVALID, "%s: container version %u, this library reads version %u", what, h.version, GDG_CKPT_VERSION);
    if (h.total_bytes > bytes)
        return fail(ctx, GDG_ERR_INVALID, "%s: the checkpoint is truncated (%zu of %llu bytes)", what, bytes, (unsigned long long)h.total_bytes);
    if (h.payload_off != sizeof(CkptHeader) || h.total_bytes < sizeof(CkptHeader) + sizeof(CkptDir) || (h.total_bytes & 15))
        return fail(ctx, GDG_ERR_INVALID, "%s: bad container sizes (payload at %u, %llu bytes)", what, h.payload_off, (unsigned long long)h.total_bytes);
    return GDG_OK;
}

/* the container staged on the device (*stage: the caller releases it, also on failure) and its digest checked there */
static int stage_verified(gdg_ctx *ctx, const char *what, const void *blob, const CkptHeader &h, unsigned char **stage) {
    HIP_TRY(ctx, ctx->arena.alloc((void **)stage, h.total_bytes));
    HIP_TRY(ctx, hipMemcpyAsync(*stage, blob, h.total_bytes, hipMemcpyHostToDevice, ctx->stream));
    uint64_t d[2] = { 0, 0 };
    const int rc = payload_digest(ctx, *stage, h.total_bytes, d);
    if (rc != GDG_OK) return rc;
    if (d[0] != h.digest[0] || d[1] != h.digest[1])
        return fail(ctx, GDG_ERR_INVALID, "%s: the payload's digest is %016llx%016llx, the container records %016llx%016llx (a damaged checkpoint)", what,
                    (unsigned long long)d[0], (unsigned long long)d[1], (unsigned long long)h.digest[0], (unsigned long long)h.digest[1]);
    return GDG_OK;
}

int gdg_state_verify(gdg_ctx *ctx, const void *blob, size_t bytes) {
    if (!ctx || !blob) return GDG_ERR_INVALID;
    CkptHeader h;
    int rc = read_header(ctx, "state verify", blob, bytes, h);
    if (rc != GDG_OK) return rc;
    enter(ctx, /*read_only=*/true);
    unsigned char *stage = nullptr;
    rc = stage_verified(ctx, "state verify", blob, h, &stage);
    hipStreamSynchronize(ctx->stream);
    ctx->arena.release(stage);
    return rc;
}

static int resume(gdg_ctx *ctx, const gdg_batch_input *inputs, int n_inputs, const gdg_batch_options *opt, bool shard, size_t job_samples,
                  bool run_metronome, const void *blob, size_t bytes, size_t *samples_done) {
    if (!ctx || !inputs || !opt || !blob || !samples_done) return GDG_ERR_INVALID;
    const char *what = shard ? "resume (shard)" : "resume";
    if (batch_sources_shared(ctx)) return SHARED_SOURCES_REFUSED(ctx, what);
    if (ctx->blend.max_reach() > 0) return BLEND_HISTORY_REFUSED(ctx, what);
    if (delivery_on(ctx)) return DELIVERY_HISTORY_REFUSED(ctx, what);
    if (ctx->out_rec_on) return OUT_RECORDS_HISTORY_REFUSED(ctx, what);
    if (const int rl = loudness_refused(ctx, what, "their state is not in the version-1 container")) return rl;
    if (ctx->bstream.open) return fail(ctx, GDG_ERR_INVALID, "%s: a streamed batch run is already open on this context", what);
    CkptHeader h;
    int rc = read_header(ctx, what, blob, bytes, h);
    if (rc != GDG_OK) return rc;
    enter(ctx, /*read_only=*/true);                   /* behind everything queued; what was made ahead stays until the checkpoint is known to fit */
    unsigned char *stage = nullptr;
    gdg_ctx::BatchStreamState job;
    auto body = [&]() -> int {
        /* 1. the digest, on the device, before anything in the payload is believed */
        int r = stage_verified(ctx, what, blob, h, &stage);
        if (r != GDG_OK) return r;
        const unsigned char *hb = static_cast<const unsigned char *>(blob);
        CkptDir dir;
        memcpy(&dir, hb + sizeof(CkptHeader), sizeof(dir));
        for (int s = 0; s < SEC_COUNT; s++) {
            const CkptSection &c = dir.s[s];
            if (c.bytes && (c.off < sizeof(CkptHeader) + sizeof(CkptDir) || (c.off & 15) || c.off > h.total_bytes || c.bytes > h.total_bytes - c.off))
                return fail(ctx, GDG_ERR_INVALID, "%s: the %s section lies outside the container", what, section_names[s]);
        }
        const size_t N = (size_t)ctx->nch;
        /* 2. the job: the one this call describes against the one recorded */
        if (dir.s[SEC_JOB].bytes < sizeof(CkptJob)) return fail(ctx, GDG_ERR_INVALID, "%s: the checkpoint holds no job", what);
        CkptJob j;
        memcpy(&j, hb + dir.s[SEC_JOB].off, sizeof(j));
        if ((j.shard != 0) != shard)
            return fail(ctx, GDG_ERR_INVALID, shard ? "%s: the checkpoint is of a plain job (gdg_batch_stream_open): gdg_batch_stream_resume continues it"
                                                    : "%s: the checkpoint is of a shard's job (gdg_batch_stream_open_shard): gdg_batch_stream_resume_shard continues it", what);
        if (j.n_inputs != (uint32_t)n_inputs || (size_t)n_inputs != N)
            return fail(ctx, GDG_ERR_INVALID, "%s: channel count: %d inputs given, the context has %d channels, the checkpoint %u", what, n_inputs, ctx->nch, j.n_inputs);
        if (dir.s[SEC_JOB].bytes != sizeof(CkptJob) + N * sizeof(CkptInput) || dir.s[SEC_CARRY].bytes != N * GDG_STREAM_CARRY * sizeof(double) ||
            dir.s[SEC_METRONOME].bytes != sizeof(CkptMetronome) || dir.s[SEC_METERS].bytes < sizeof(CkptMeterHead) || !dir.s[SEC_STATE].bytes)
            return fail(ctx, GDG_ERR_INVALID, "%s: a section of the checkpoint has the wrong size for %zu channels", what, N);
        if ((r = stream_job(ctx, inputs, n_inputs, opt, shard, job_samples, run_metronome, job)) != GDG_OK) return r;
#define JOB_MISMATCH(name, fmt, here, there) \
    return fail(ctx, GDG_ERR_INVALID, "%s: " name ": " fmt " given, " fmt " in the checkpoint", what, here, there)
        if (j.target_rate != opt->target_rate) JOB_MISMATCH("target_rate", "%u", opt->target_rate, j.target_rate);
        if (j.out_format != opt->out_format) JOB_MISMATCH("out_format", "%d", opt->out_format, j.out_format);
        if (j.metronome_to_master != (opt->metronome_to_master != 0)) JOB_MISMATCH("metronome_to_master", "%d", opt->metronome_to_master != 0, j.metronome_to_master);
        if (j.run_meters != (opt->run_meters != 0)) JOB_MISMATCH("run_meters", "%d", opt->run_meters != 0, j.run_meters);
        if (j.tuner_enqueue != (opt->tuner_enqueue != 0)) JOB_MISMATCH("tuner_enqueue", "%d", opt->tuner_enqueue != 0, j.tuner_enqueue);
        if (shard && (j.run_metronome != 0) != run_metronome) JOB_MISMATCH("run_metronome", "%d", (int)run_metronome, (int)j.run_metronome);
        std::vector<CkptInput> rec(N);
        memcpy(rec.data(), hb + dir.s[SEC_JOB].off + sizeof(j), N * sizeof(CkptInput));
        for (size_t i = 0; i < N; i++) {
            const gdg_batch_input &in = inputs[i];
            const CkptInput &c = rec[i];
#define INPUT_MISMATCH(field, here, there) \
    return fail(ctx, GDG_ERR_INVALID, "%s: input %zu: " field ": %llu given, %llu in the checkpoint", what, i, (unsigned long long)(here), (unsigned long long)(there))
            if (input_has_samples(in) != (c.has_samples != 0)) INPUT_MISMATCH("has samples", input_has_samples(in), c.has_samples);
            if (c.has_samples) {
                if (in.samples_per_channel != c.samples_per_channel) INPUT_MISMATCH("samples_per_channel", in.samples_per_channel, c.samples_per_channel);
                if (in.format != c.format) INPUT_MISMATCH("format", in.format, c.format);
                if (in.sample_rate != c.sample_rate) INPUT_MISMATCH("sample rate", in.sample_rate, c.sample_rate);
                if (in.channels != c.channels) INPUT_MISMATCH("channels", in.channels, c.channels);
                if (in.channel != c.channel) INPUT_MISMATCH("channel", in.channel, c.channel);
            }
            if (job.n_out[i] != c.n_out) INPUT_MISMATCH("samples covered", job.n_out[i], c.n_out);
            if (c.brought > (c.has_samples ? c.samples_per_channel : 0)) INPUT_MISMATCH("frames handed over", 0, c.brought);
            job.brought[i] = (size_t)c.brought;
        }
#undef INPUT_MISMATCH
        if (job.length != j.length) JOB_MISMATCH("length (a shard: job_samples)", "%llu", (unsigned long long)job.length, (unsigned long long)j.length);
        if (j.pos > j.length || j.pos % GDG_BLOCK_SIZE) JOB_MISMATCH("position", "%llu", 0ull, (unsigned long long)j.pos);
#undef JOB_MISMATCH
        job.pos = (size_t)j.pos;
        for (size_t i = 0; i < N; i++)
            if (rec[i].carry_valid != carry_valid(job, i))
                return fail(ctx, GDG_ERR_INVALID, "%s: input %zu: %u carried frames recorded, its position keeps %u", what, i, rec[i].carry_valid, carry_valid(job, i));
        /* 3. every layout key of the embedded channel state, as gdg_state_load checks it before it touches anything */
        if ((r = state_check_device(ctx, stage + dir.s[SEC_STATE].off, (size_t)dir.s[SEC_STATE].bytes)) != GDG_OK) return r;
        /* 4. meters and tuner */
        CkptMeterHead mh;
        memcpy(&mh, hb + dir.s[SEC_METERS].off, sizeof(mh));
        if (mh.ports != (uint32_t)ctx->n_meter || mh.record_bytes != sizeof(gdg_meter_rec) ||
            dir.s[SEC_METERS].bytes != sizeof(mh) + (size_t)mh.ports * sizeof(gdg_meter_rec))
            return fail(ctx, GDG_ERR_INVALID, "%s: meter ports: %d configured here (gdg_meter_configure), %u in the checkpoint", what, ctx->n_meter, mh.ports);
        CkptTunerHead th = { 0, 0, 0, 0 };
        const bool rings = dir.s[SEC_TUNER].bytes != 0;
        if (rings) {
            if (dir.s[SEC_TUNER].bytes < sizeof(th)) return fail(ctx, GDG_ERR_INVALID, "%s: the tuner section is cut short", what);
            memcpy(&th, hb + dir.s[SEC_TUNER].off, sizeof(th));
            if (th.ring_len != GDG_TUNER_RING || th.channels != (uint32_t)N || dir.s[SEC_TUNER].bytes != sizeof(th) + N * GDG_TUNER_RING * sizeof(double))
                return fail(ctx, GDG_ERR_INVALID, "%s: tuner rings: %d samples for each of %zu channels here, %u for %u in the checkpoint", what,
                            GDG_TUNER_RING, N, th.ring_len, th.channels);
        }
        CkptMetronome m;
        memcpy(&m, hb + dir.s[SEC_METRONOME].off, sizeof(m));
        /* 5. everything fits: the buffers the pieces land in, then ONE launch for the channel state and all the rest */
        double *d_carry = nullptr;
        if ((r = batch_carry_buffer(ctx, &d_carry)) != GDG_OK) return r;
        if (rings && (r = ensure_tuner(ctx)) != GDG_OK) return r;
        Pieces extra;
        extra.add(stage + dir.s[SEC_CARRY].off, d_carry, N * GDG_STREAM_CARRY * sizeof(double));
        for (int p = 0; p < ctx->n_meter; p++)                   /* value, held peak, hold counter; the enabled flag is the target's configuration */
            extra.add(stage + dir.s[SEC_METERS].off + sizeof(mh) + (size_t)p * sizeof(gdg_meter_rec), ctx->d_meter + p, offsetof(gdg_meter_rec, enabled));
        if (rings) extra.add(stage + dir.s[SEC_TUNER].off + sizeof(th), ctx->d_tuner_ring, N * GDG_TUNER_RING * sizeof(double));
        else if (ctx->d_tuner_ring) extra.add(nullptr, ctx->d_tuner_ring, N * GDG_TUNER_RING * sizeof(double));      /* the source never fed a tuner */
        if ((r = state_load_device_with(ctx, stage + dir.s[SEC_STATE].off, (size_t)dir.s[SEC_STATE].bytes, &extra)) != GDG_OK) return r;
        ctx->tuner_wp = 0;                                       /* the rings came oldest sample first */
        if (rings || ctx->d_tuner_ring) ctx->tuner_sr = th.rate;
        ctx->met_sample_counter = m.sample_counter;
        ctx->met_tick_counter = m.tick_counter;
        return GDG_OK;
    };
    rc = body();
    hipStreamSynchronize(ctx->stream);
    ctx->arena.release(stage);
    if (rc != GDG_OK) return rc;
    ctx->bstream = job;
    *samples_done = job.pos;
    return GDG_OK;
}

int gdg_batch_stream_resume(gdg_ctx *ctx, const gdg_batch_input *inputs, int n_inputs, const gdg_batch_options *options, const void *blob,
                            size_t bytes, size_t *samples_done) {
    return resume(ctx, inputs, n_inputs, options, false, 0, true, blob, bytes, samples_done);
}

int gdg_batch_stream_resume_shard(gdg_ctx *ctx, const gdg_batch_input *inputs, int n_inputs, const gdg_batch_options *options, size_t job_samples,
                                  int run_metronome, const void *blob, size_t bytes, size_t *samples_done) {
    if (ctx && ctx->blend.count())
        return fail(ctx, GDG_ERR_UNSUPPORTED, "gdg_batch_stream_resume_shard: %d blends are in force on this context (gdg_batch_set_blends); a sharded job cannot write blend outputs yet",
                    ctx->blend.count());
    if (const int rc = lists_refused(ctx, "gdg_batch_stream_resume_shard")) return rc;
    if (ctx && options && options->metronome_to_master)
        return fail(ctx, GDG_ERR_INVALID, "gdg_batch_stream_resume_shard: metronome_to_master must be 0, as for gdg_batch_stream_open_shard");
    return resume(ctx, inputs, n_inputs, options, true, job_samples, run_metronome != 0, blob, bytes, samples_done);
}
