/*
 * api_state.cpp -- channel state out of a context and into another one (gdg_state_*; include/gdg.h documents the format and its rules).
 * Part of the host side of libgdg.so (the C-ABI of include/gdg.h on top of the HIP kernels; see ctx.h for the map).
 *
 * A save or a load is a list of contiguous pieces {src, dst, bytes} -- one per state region, one per delay-line slot -- that ONE launch of
 * state.hip's copy kernel moves on the context's stream.  The host side only decides addresses: the blob's metadata (header, per channel a
 * record and its slot table) is built here, the payload never passes through the host except in the host-buffer calls' one copy.
 */
#include "ctx.h"

#define GDG_STATE_MAGIC "GDGSTATE"
#define GDG_STATE_VERSION 1u

enum { SLOT_BYPASS = 1, SLOT_FRESH = 2, SLOT_FIR = 4 };

/* little-endian, natural alignment, no padding the compiler adds (static_asserts below) */
struct StateHeader {
    char magic[8];
    uint32_t version, count;          /* format version, records (channels) */
    int32_t frames;                   /* the frame size the state was laid out for (0: no plan was ever built, every slot is fresh) */
    uint32_t rate;                    /* ... and the sample rate */
    int32_t max_frames;               /* the source context's */
    uint32_t meta_bytes;              /* header + records + slot tables, rounded up to 16: the payload starts here */
    uint64_t total_bytes;
    uint32_t reserved[6];
};
struct StateRecord {
    int32_t channel, n_slots;         /* the source channel (informative), slots of its chain */
    uint32_t sp_len, sp_sr;           /* spatializer history row: samples (0: the source had none) and the rate it was made for */
    uint64_t sp_off;
    uint64_t reserved;
};
struct StateSlot {
    int32_t type, flags;              /* unit type; SLOT_* */
    int64_t hist_key;                 /* the ring layout: what it was built for, its length in doubles */
    uint64_t hist_len;
    int32_t os_frames[2];             /* frame size the 2x / 4x oversampler last saw (-1: never made) */
    int32_t bp_half_order;
    int32_t fir_P, fir_K, fir_hop;    /* SLOT_FIR: the delay line's transform half size, partitions, frame size */
    uint32_t fir_sr;
    int32_t fir_pos;                  /* ... and the frame counter: slot m of the payload is frame fir_pos - 1 - m */
    uint64_t off_ds, off_is, off_hist, off_prev, off_fdl;      /* payload offsets from the blob's start (0: not present) */
};
static_assert(sizeof(StateHeader) == 64, "blob header layout");
static_assert(sizeof(StateRecord) == 32, "blob record layout");
static_assert(sizeof(StateSlot) == 96, "blob slot layout");

/* which oversampler (0: 2x, 1: 4x) the unit's parameters use, -1 none */
static int os_in_use(const Unit &u) {
    int idx = -1;
    if (shaper_os_param(u.type) >= 0) idx = u.params[shaper_os_param(u.type)];
    else if (u.type == GDG_UNIT_FUZZ) idx = u.params[6];
    return idx == 1 ? 0 : idx == 2 ? 1 : -1;
}

static const char *unit_type_name(int type) {
    static const char *const names[GDG_UNIT_COUNT] = {                 /* include/gdg.h's order */
        "signal generator", "noise gate", "bandpass", "auto-wah", "auto-yoy", "compressor", "octaver", "excess", "fuzz", "overdrive",
        "distortion", "tone stack", "chorus", "flanger", "phaser", "tremolo", "ring modulator", "delay", "reverb", "power amp", "cabinet" };
    return (type >= 0 && type < GDG_UNIT_COUNT) ? names[type] : "?";
}

static int channel_list(gdg_ctx *ctx, const int *channels, int n, std::vector<int> &out) {
    out.clear();
    if (!channels) {
        for (int c = 0; c < ctx->nch; c++) out.push_back(c);
        return GDG_OK;
    }
    if (n < 0) return fail(ctx, GDG_ERR_INVALID, "state: %d channels", n);
    std::vector<char> seen((size_t)ctx->nch, 0);
    for (int i = 0; i < n; i++) {
        const int c = channels[i];
        if (c < 0 || c >= ctx->nch) return fail(ctx, GDG_ERR_INVALID, "state: channel %d out of range (%d channels)", c, ctx->nch);
        if (seen[(size_t)c]) return fail(ctx, GDG_ERR_INVALID, "state: channel %d listed twice", c);
        seen[(size_t)c] = 1;
        out.push_back(c);
    }
    return GDG_OK;
}

/* The metadata of a save of `chans` (pos fields still 0) and the blob's size.  Everything in it comes from host fields. */
static void layout(const gdg_ctx *ctx, const std::vector<int> &chans, std::vector<unsigned char> &meta, size_t &total) {
    size_t n_slots = 0;
    for (int c : chans) n_slots += ctx->chains[(size_t)c].size();
    const size_t meta_bytes = round16(sizeof(StateHeader) + chans.size() * sizeof(StateRecord) + n_slots * sizeof(StateSlot));
    meta.assign(meta_bytes, 0);
    StateHeader h;
    memset(&h, 0, sizeof(h));
    memcpy(h.magic, GDG_STATE_MAGIC, 8);
    h.version = GDG_STATE_VERSION;
    h.count = (uint32_t)chans.size();
    h.frames = ctx->plan_frames;
    h.rate = ctx->plan_sr;
    h.max_frames = ctx->max_frames;
    h.meta_bytes = (uint32_t)meta_bytes;
    size_t at = sizeof(StateHeader), off = meta_bytes;
    for (int c : chans) {
        const auto &chain = ctx->chains[(size_t)c];
        StateRecord r;
        memset(&r, 0, sizeof(r));
        r.channel = c;
        r.n_slots = (int32_t)chain.size();
        for (const Slot &s : chain) {
            const Unit &u = ctx->units[(size_t)s.handle];
            StateSlot t;
            memset(&t, 0, sizeof(t));
            t.type = u.type;
            t.hist_key = u.hist_key;
            t.hist_len = u.hist_len;
            t.os_frames[0] = u.os_frames[0]; t.os_frames[1] = u.os_frames[1];
            t.bp_half_order = u.bp_half_order;
            t.flags = s.bypass ? SLOT_BYPASS : 0;
            const bool fir = u.type == GDG_UNIT_POWERAMP;
            if (fir ? !u.fir_live : !u.ran) {
                t.flags |= SLOT_FRESH;
            } else {
                t.off_ds = off; off += GDG_DS_LEN * sizeof(double);
                t.off_is = off; off += round16(GDG_IS_LEN * sizeof(int));
                if (u.d_hist && u.hist_len) { t.off_hist = off; off += round16(u.hist_len * sizeof(double)); }
                if (fir) {
                    t.flags |= SLOT_FIR;
                    t.fir_P = u.fir_P; t.fir_K = u.fir_K; t.fir_hop = u.fir_hop; t.fir_sr = u.fir_sr;
                    t.off_prev = off; off += 2 * (size_t)u.fir_P * sizeof(double);
                    t.off_fdl = off; off += (size_t)u.fir_K * (size_t)u.fir_P * sizeof(double2);
                }
            }
            memcpy(&meta[at + sizeof(StateRecord) + (&s - chain.data()) * sizeof(StateSlot)], &t, sizeof(t));
        }
        if (ctx->d_sp_hist) {
            r.sp_len = (uint32_t)ctx->sp_hist_len;
            r.sp_sr = ctx->sp_hist_sr;
            r.sp_off = off;
            off += round16((size_t)ctx->sp_hist_len * sizeof(double));
        }
        memcpy(&meta[at], &r, sizeof(r));
        at += sizeof(StateRecord) + chain.size() * sizeof(StateSlot);
    }
    total = off;
    h.total_bytes = total;
    memcpy(meta.data(), &h, sizeof(h));
}

static inline int ring_slot(int pos, int m, int R) { return (((pos - 1 - m) % R) + R) % R; }      /* frame pos - 1 - m (prepare_fir) */

int gdg_state_size(gdg_ctx *ctx, const int *channels, int n, size_t *bytes) {
    if (!ctx || !bytes) return GDG_ERR_INVALID;
    std::vector<int> chans;
    int rc = channel_list(ctx, channels, n, chans);
    if (rc != GDG_OK) return rc;
    std::vector<unsigned char> meta;
    layout(ctx, chans, meta, *bytes);
    return GDG_OK;
}

/* blob: the caller's device buffer, or staging in the arena */
static int save_into(gdg_ctx *ctx, const std::vector<int> &chans, unsigned char *blob, const std::vector<unsigned char> &meta_in, const Pieces *extra = nullptr) {
    std::vector<unsigned char> meta = meta_in;
    /* 1. the frame counters of the live delay lines: the ring rotation is decided on the host */
    std::vector<std::pair<size_t, const Unit *>> firs;          /* (offset of the slot in meta, unit) */
    size_t at = sizeof(StateHeader);
    for (int c : chans) {
        const auto &chain = ctx->chains[(size_t)c];
        for (size_t i = 0; i < chain.size(); i++) {
            const size_t so = at + sizeof(StateRecord) + i * sizeof(StateSlot);
            StateSlot t;
            memcpy(&t, &meta[so], sizeof(t));
            if (t.flags & SLOT_FIR) firs.emplace_back(so, &ctx->units[(size_t)chain[i].handle]);
        }
        at += sizeof(StateRecord) + chain.size() * sizeof(StateSlot);
    }
    std::vector<int> pos(firs.size(), 0);
    if (!firs.empty()) {
        int *d_pos = nullptr;
        HIP_TRY(ctx, ctx->arena.alloc((void **)&d_pos, firs.size() * sizeof(int)));
        Pieces g;
        for (size_t i = 0; i < firs.size(); i++) g.add(firs[i].second->d_pos, d_pos + i, sizeof(int));
        int rc = g.run(ctx);
        hipError_t e = rc == GDG_OK ? hipMemcpy(pos.data(), d_pos, pos.size() * sizeof(int), hipMemcpyDeviceToHost) : hipSuccess;
        ctx->arena.release(d_pos);
        if (rc != GDG_OK) return rc;
        if (e != hipSuccess) return fail(ctx, GDG_ERR_HIP, "state save: %s", hipGetErrorString(e));
        for (size_t i = 0; i < firs.size(); i++) {
            StateSlot t;
            memcpy(&t, &meta[firs[i].first], sizeof(t));
            t.fir_pos = pos[i];
            memcpy(&meta[firs[i].first], &t, sizeof(t));
        }
    }
    /* 2. the metadata, then every region in one launch */
    HIP_TRY(ctx, hipMemcpyAsync(blob, meta.data(), meta.size(), hipMemcpyHostToDevice, ctx->stream));
    Pieces ps;
    at = sizeof(StateHeader);
    for (int c : chans) {
        const auto &chain = ctx->chains[(size_t)c];
        StateRecord r;
        memcpy(&r, &meta[at], sizeof(r));
        for (size_t i = 0; i < chain.size(); i++) {
            StateSlot t;
            memcpy(&t, &meta[at + sizeof(StateRecord) + i * sizeof(StateSlot)], sizeof(t));
            if (t.flags & SLOT_FRESH) continue;
            const Unit &u = ctx->units[(size_t)chain[i].handle];
            ps.add(u.d_ds, blob + t.off_ds, GDG_DS_LEN * sizeof(double));
            ps.add_padded(u.d_is, blob + t.off_is, GDG_IS_LEN * sizeof(int), true);
            if (t.off_hist) ps.add_padded(u.d_hist, blob + t.off_hist, u.hist_len * sizeof(double), true);
            if (t.flags & SLOT_FIR) {
                ps.add(u.d_prev, blob + t.off_prev, 2 * (size_t)u.fir_P * sizeof(double));
                const size_t slot_bytes = (size_t)u.fir_P * sizeof(double2);
                for (int m = 0; m < u.fir_K; m++)          /* age order: the newest frame first */
                    ps.add(u.d_fdl + (size_t)ring_slot(t.fir_pos, m, u.fir_R) * u.fir_P, blob + t.off_fdl + (size_t)m * slot_bytes, slot_bytes);
            }
        }
        if (r.sp_len) {
            const double *row = ctx->d_sp_hist + (size_t)ctx->sp_hist_cur * (size_t)ctx->nch * r.sp_len + (size_t)c * r.sp_len;
            ps.add_padded(row, blob + r.sp_off, (size_t)r.sp_len * sizeof(double), true);
        }
        at += sizeof(StateRecord) + chain.size() * sizeof(StateSlot);
    }
    ps.append(extra);
    return ps.run(ctx);
}

static int save_common(gdg_ctx *ctx, const int *channels, int n, void *blob, size_t capacity, size_t *written, bool device, const Pieces *extra = nullptr) {
    if (!ctx || !blob) return GDG_ERR_INVALID;
    std::vector<int> chans;
    int rc = channel_list(ctx, channels, n, chans);
    if (rc != GDG_OK) return rc;
    std::vector<unsigned char> meta;
    size_t total = 0;
    layout(ctx, chans, meta, total);
    if (written) *written = total;
    if (capacity < total) return fail(ctx, GDG_ERR_INVALID, "state save: %zu bytes of capacity, the state of %zu channels takes %zu (gdg_state_size)", capacity, chans.size(), total);
    if (device && ((uintptr_t)blob & 15)) return fail(ctx, GDG_ERR_INVALID, "state save: the device buffer must be 16-byte aligned");
    /* ordered after everything queued on the context; nothing it made ahead is dropped (a save changes no state) */
    enter(ctx, /*read_only=*/true);
    if (device) return save_into(ctx, chans, static_cast<unsigned char *>(blob), meta, extra);
    unsigned char *stage = nullptr;
    HIP_TRY(ctx, ctx->arena.alloc((void **)&stage, total));
    rc = save_into(ctx, chans, stage, meta);
    if (rc == GDG_OK) {
        hipError_t e = hipMemcpy(blob, stage, total, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(ctx, GDG_ERR_HIP, "state save: %s", hipGetErrorString(e));
    }
    hipStreamSynchronize(ctx->stream);
    ctx->arena.release(stage);
    return rc;
}

int gdg_state_save(gdg_ctx *ctx, const int *channels, int n, void *blob, size_t capacity, size_t *written) {
    return save_common(ctx, channels, n, blob, capacity, written, false);
}
int gdg_state_save_device(gdg_ctx *ctx, const int *channels, int n, void *d_blob, size_t capacity, size_t *written) {
    return save_common(ctx, channels, n, d_blob, capacity, written, true);
}

/* ---- load ------------------------------------------------------------------------------------------------------------------------ */

/* What a load lays out: every unit in the chain that is not bypassed (a process call would), and bypassed ones that were never laid out
 * (nothing of theirs can change). */
static bool lays_out(const Unit &u, bool bypass) {
    if (!bypass) return true;
    return u.type == GDG_UNIT_POWERAMP ? !u.fir_live : !u.ran;
}

/* The layout keys of a unit: as it stands (built = true), or as prepare_unit / prepare_fir (api_plan.cpp) WILL leave it at `frames` and
 * `rate` when the load lays it out.  Only reads: a rejected load must find the target as it was.  The formulas are prepare_unit's;
 * the load checks the built layout against the blob again afterwards. */
struct Layout { long long hist_key; size_t hist_len; int os_frames[2]; int bp_half_order; int P, K, hop; uint32_t sr; bool fir_built; };
static Layout unit_layout(const gdg_ctx *ctx, const Unit &u, bool bypass, int frames, uint32_t rate, bool built) {
    Layout e = { u.hist_key, u.hist_len, { u.os_frames[0], u.os_frames[1] }, u.bp_half_order, u.fir_P, u.fir_K, u.fir_hop, u.fir_sr,
                 !u.fir_dirty && u.d_fdl != nullptr };
    if (built || frames <= 0 || !lays_out(u, bypass)) return e;
    const double sr = (double)rate;
    const int32_t *p = u.params;
    switch (u.type) {
    case GDG_UNIT_OVERDRIVE: case GDG_UNIT_DISTORTION: case GDG_UNIT_EXCESS: case GDG_UNIT_FUZZ: {
        const int w = os_in_use(u);
        if (w >= 0) { e.hist_key = 1; e.hist_len = (8 + 76) + (8 + 154); e.os_frames[w] = frames; }
        break;
    }
    case GDG_UNIT_CHORUS: {
        const int C = (int)floor((0.05 * sr) + 0.5);
        size_t cp = 1;
        while (cp < (size_t)C + (size_t)ctx->max_frames) cp <<= 1;
        e.hist_key = C; e.hist_len = cp + 1;
        break;
    }
    case GDG_UNIT_FLANGER: case GDG_UNIT_PHASER: {
        const int C = (int)floor((0.002 * sr) + 0.5);
        e.hist_key = C; e.hist_len = (size_t)C;
        break;
    }
    case GDG_UNIT_DELAY: {
        const int D = (int)floor(((0.001 * (double)p[0]) * sr) + 0.5);
        e.hist_key = D; e.hist_len = (size_t)D;
        break;
    }
    case GDG_UNIT_AUTOYOY: {
        const int C = (int)floor((0.01 * sr) + 0.5);
        e.hist_key = C; e.hist_len = (size_t)C;
        break;
    }
    case GDG_UNIT_REVERB: {
        static const double ap_delays[3] = { 0.04204, 0.01348, 0.00452 };
        static const double tap_times[4] = { 0.19196, 0.19996, 0.21596, 0.23204 };
        uint32_t max_index = 0;
        for (int i = 0; i < 4; i++) max_index = std::max(max_index, (uint32_t)round(tap_times[i] * sr));
        size_t len = (size_t)max_index + GDG_MAX_FRAMES;
        for (int i = 0; i < 3; i++) { const int D = (int)round(ap_delays[i] * sr); len += (size_t)(D > 1 ? D - 1 : 0); }
        e.hist_key = (long long)rate; e.hist_len = ((len + 1) & ~(size_t)1) + GDG_MAX_FRAMES;
        break;
    }
    case GDG_UNIT_BANDPASS: {
        static const int orders[4] = { 2, 4, 6, 8 };
        e.bp_half_order = (p[0] >= 0 && p[0] < 4) ? orders[p[0]] >> 1 : 0;
        break;
    }
    case GDG_UNIT_POWERAMP: {
        const int L = (int)u.taps.size();
        e.P = fir_transform_size(frames);
        e.K = std::max(1, (L + frames - 1) / frames);
        e.hop = frames; e.sr = rate; e.fir_built = true;
        break;
    }
    default: break;
    }
    return e;
}

/* Every non-fresh slot's keys against the target's layout (as it will be: built = false; as it is: built = true) */
static int check_all(gdg_ctx *ctx, const std::vector<int> &chans, const std::vector<unsigned char> &meta, const StateHeader &h, bool built) {
    size_t at = sizeof(StateHeader);
    for (size_t i = 0; i < chans.size(); i++) {
        const int c = chans[i];
        StateRecord r;
        memcpy(&r, &meta[at], sizeof(r));
        const auto &chain = ctx->chains[(size_t)c];
        for (size_t s = 0; s < chain.size(); s++) {
            StateSlot t;
            memcpy(&t, &meta[at + sizeof(r) + s * sizeof(t)], sizeof(t));
            if (t.flags & SLOT_FRESH) continue;
            const Unit &u = ctx->units[(size_t)chain[s].handle];
            const Layout e = unit_layout(ctx, u, chain[s].bypass, h.frames, h.rate, built);
            const char *tn = unit_type_name(u.type);
#define KEY_MISMATCH(key, fmt, here, blob) \
    return fail(ctx, GDG_ERR_INVALID, "state load: channel %d slot %zu (%s): " key " " fmt " here, " fmt " in the blob", c, s, tn, here, blob)
            if (t.hist_key != e.hist_key) KEY_MISMATCH("hist_key", "%lld", (long long)e.hist_key, (long long)t.hist_key);
            if (t.hist_len != e.hist_len) KEY_MISMATCH("hist_len", "%zu", (size_t)e.hist_len, (size_t)t.hist_len);
            if (built && t.off_hist && !u.d_hist) KEY_MISMATCH("hist_len", "%zu", (size_t)0, (size_t)t.hist_len);
            const int w = os_in_use(u);
            if (w >= 0 && !chain[s].bypass && t.os_frames[w] != e.os_frames[w])
                KEY_MISMATCH("oversampler frames", "%d", e.os_frames[w], t.os_frames[w]);
            if (u.type == GDG_UNIT_BANDPASS && e.bp_half_order >= 0 && t.bp_half_order != e.bp_half_order)
                KEY_MISMATCH("bandpass half order", "%d", e.bp_half_order, t.bp_half_order);
            if (u.type == GDG_UNIT_POWERAMP) {
                if (!(t.flags & SLOT_FIR)) KEY_MISMATCH("filter", "%s", "live", "none");
                if (!e.fir_built) KEY_MISMATCH("filter", "%s", "not built", "live");
                if (t.fir_P != e.P) KEY_MISMATCH("P", "%d", e.P, t.fir_P);
                if (t.fir_K != e.K) KEY_MISMATCH("K", "%d", e.K, t.fir_K);
                if (t.fir_hop != e.hop) KEY_MISMATCH("hop", "%d", e.hop, t.fir_hop);
                if (t.fir_sr != e.sr) KEY_MISMATCH("sample rate", "%u", e.sr, t.fir_sr);
            } else if (t.flags & SLOT_FIR) {
                KEY_MISMATCH("filter", "%s", "none", "live");
            }
#undef KEY_MISMATCH
        }
        if (r.sp_len) {
            if (ctx->d_sp_hist && (ctx->sp_hist_sr != r.sp_sr || (uint32_t)ctx->sp_hist_len != r.sp_len))
                return fail(ctx, GDG_ERR_INVALID, "state load: channel %d: spatializer history of %d samples at %u Hz here, %u at %u Hz in the blob", c,
                            ctx->sp_hist_len, ctx->sp_hist_sr, r.sp_len, r.sp_sr);
            if (!ctx->d_sp_hist && r.sp_sr != ctx->sp_hist_sr)
                return fail(ctx, GDG_ERR_INVALID, "state load: channel %d: spatializer rate %u Hz here, %u Hz in the blob", c, ctx->sp_hist_sr, r.sp_sr);
        }
        at += sizeof(r) + chain.size() * sizeof(StateSlot);
    }
    return GDG_OK;
}

/* The metadata against the target: structure and every layout key first, against the layouts the load will build (nothing touched, the
 * sums made ahead kept); then the target's layouts at the blob's frame size and rate, and the keys once more.  GDG_OK: the blob can be
 * applied as it is. */
static int validate(gdg_ctx *ctx, const std::vector<int> &chans, const std::vector<unsigned char> &meta, const StateHeader &h, bool check_only = false) {
    size_t at = sizeof(StateHeader);
    /* 1. structure: records, slot counts, unit types, offsets inside the blob */
    for (size_t i = 0; i < chans.size(); i++) {
        const int c = chans[i];
        StateRecord r;
        if (at + sizeof(r) > h.meta_bytes) return fail(ctx, GDG_ERR_INVALID, "state load: the blob's metadata ends in record %zu", i);
        memcpy(&r, &meta[at], sizeof(r));
        const auto &chain = ctx->chains[(size_t)c];
        if (r.n_slots < 0 || at + sizeof(r) + (size_t)r.n_slots * sizeof(StateSlot) > h.meta_bytes)
            return fail(ctx, GDG_ERR_INVALID, "state load: record %zu (channel %d) runs past the blob's metadata", i, c);
        if ((size_t)r.n_slots != chain.size())
            return fail(ctx, GDG_ERR_INVALID, "state load: channel %d has %zu slots, record %zu of the blob %d", c, chain.size(), i, r.n_slots);
        for (size_t s = 0; s < chain.size(); s++) {
            StateSlot t;
            memcpy(&t, &meta[at + sizeof(r) + s * sizeof(t)], sizeof(t));
            const Unit &u = ctx->units[(size_t)chain[s].handle];
            if (t.type != u.type)
                return fail(ctx, GDG_ERR_INVALID, "state load: channel %d slot %zu: unit type %s (%d) here, %s (%d) in the blob", c, s,
                            unit_type_name(u.type), u.type, unit_type_name(t.type), t.type);
            if (t.flags & SLOT_FRESH) continue;
            const size_t fir_bytes = (t.flags & SLOT_FIR) ? 2 * (size_t)t.fir_P * sizeof(double) + (size_t)t.fir_K * (size_t)t.fir_P * sizeof(double2) : 0;
            const bool bad_off = t.off_ds < h.meta_bytes || t.off_ds + GDG_DS_LEN * sizeof(double) > h.total_bytes ||
                                 t.off_is + GDG_IS_LEN * sizeof(int) > h.total_bytes ||
                                 (t.off_hist && t.off_hist + t.hist_len * sizeof(double) > h.total_bytes) ||
                                 ((t.flags & SLOT_FIR) && (t.fir_P <= 0 || t.fir_K <= 0 || t.off_prev + fir_bytes > h.total_bytes ||
                                                           t.off_fdl + (size_t)t.fir_K * (size_t)t.fir_P * sizeof(double2) > h.total_bytes)) ||
                                 ((t.off_ds | t.off_is | t.off_hist | t.off_prev | t.off_fdl) & 15);
            if (bad_off) return fail(ctx, GDG_ERR_INVALID, "state load: channel %d slot %zu (%s): payload offsets outside the blob", c, s, unit_type_name(u.type));
            if (h.frames <= 0) return fail(ctx, GDG_ERR_INVALID, "state load: channel %d slot %zu (%s) holds state but the blob has no frame size", c, s, unit_type_name(u.type));
        }
        if (r.sp_len && (r.sp_off < h.meta_bytes || (r.sp_off & 7) || r.sp_off + (size_t)r.sp_len * sizeof(double) > h.total_bytes))
            return fail(ctx, GDG_ERR_INVALID, "state load: record %zu (channel %d): spatializer row outside the blob", i, c);
        at += sizeof(r) + chain.size() * sizeof(StateSlot);
    }
    if (h.frames > ctx->max_frames)
        return fail(ctx, GDG_ERR_INVALID, "state load: the blob was laid out for %d-sample frames, this context takes at most %d", h.frames, ctx->max_frames);
    /* 2. the keys against the layouts the target WILL have (expected_layout): nothing of the target is touched before every record fits */
    int rc = check_all(ctx, chans, meta, h, false);
    if (rc != GDG_OK || check_only) return rc;
    /* 3. the target's layouts at the blob's frame size and rate, built as a process call would build them; the sums made ahead die here */
    enter(ctx);
    if (h.frames > 0) {
        for (int c : chans)
            for (const Slot &s : ctx->chains[(size_t)c]) {
                Unit &u = ctx->units[(size_t)s.handle];
                if (!lays_out(u, s.bypass)) continue;
                if (u.type == GDG_UNIT_POWERAMP) {
                    rc = prepare_fir(ctx, u, h.frames, h.rate);
                } else {
                    gdg_seg_unit d;
                    rc = prepare_unit(ctx, u, h.frames, h.rate, d);
                }
                if (rc != GDG_OK) return rc;
            }
        ctx->dirty = true;
    }
    /* 4. the same keys against what was built (expected_layout follows prepare_unit / prepare_fir; a difference is a bug, reported) */
    return check_all(ctx, chans, meta, h, true);
}

/* blob: the blob on the device (the caller's buffer or staging), meta: its metadata on the host */
static int apply(gdg_ctx *ctx, const std::vector<int> &chans, const unsigned char *blob, const std::vector<unsigned char> &meta, const Pieces *extra = nullptr) {
    bool any_sp = false;
    size_t at = sizeof(StateHeader);
    for (size_t i = 0; i < chans.size(); i++) {
        StateRecord r;
        memcpy(&r, &meta[at], sizeof(r));
        any_sp |= r.sp_len != 0;
        at += sizeof(r) + (size_t)r.n_slots * sizeof(StateSlot);
    }
    if (any_sp) { int rc = ensure_spatializer(ctx); if (rc != GDG_OK) return rc; }
    Pieces ps;
    at = sizeof(StateHeader);
    for (int c : chans) {
        const auto &chain = ctx->chains[(size_t)c];
        StateRecord r;
        memcpy(&r, &meta[at], sizeof(r));
        for (size_t s = 0; s < chain.size(); s++) {
            const size_t so = at + sizeof(r) + s * sizeof(StateSlot);
            StateSlot t;
            memcpy(&t, &meta[so], sizeof(t));
            Unit &u = ctx->units[(size_t)chain[s].handle];
            if (t.flags & SLOT_FRESH) {
                /* never ran in the source: a reset (gdg_unit_reset) */
                ps.add(nullptr, u.d_ds, GDG_DS_LEN * sizeof(double));
                ps.add(nullptr, u.d_is, GDG_IS_LEN * sizeof(int));
                if (u.d_hist) ps.add(nullptr, u.d_hist, u.hist_len * sizeof(double));
                if (u.type == GDG_UNIT_POWERAMP) { u.fir_dirty = true; u.fir_live = false; }
                continue;
            }
            ps.add(blob + t.off_ds, u.d_ds, GDG_DS_LEN * sizeof(double));
            ps.add(blob + t.off_is, u.d_is, GDG_IS_LEN * sizeof(int));
            if (u.d_hist) {
                if (t.off_hist) ps.add(blob + t.off_hist, u.d_hist, u.hist_len * sizeof(double));
                else ps.add(nullptr, u.d_hist, u.hist_len * sizeof(double));
            }
            u.os_frames[0] = t.os_frames[0]; u.os_frames[1] = t.os_frames[1];
            u.bp_half_order = t.bp_half_order;
            u.ran = true;
            if (t.flags & SLOT_FIR) {
                ps.add(blob + t.off_prev, u.d_prev, 2 * (size_t)u.fir_P * sizeof(double));
                const size_t slot_bytes = (size_t)u.fir_P * sizeof(double2);
                for (int m = 0; m < u.fir_K; m++)          /* rotated into this context's ring (R = K + window - 1) */
                    ps.add(blob + t.off_fdl + (size_t)m * slot_bytes, u.d_fdl + (size_t)ring_slot(t.fir_pos, m, u.fir_R) * u.fir_P, slot_bytes);
                ps.add(blob + so + offsetof(StateSlot, fir_pos), u.d_pos, sizeof(int));
                ps.add(nullptr, u.d_pos + 1, 3 * sizeof(int));           /* no sums made ahead: stamp (frame, epoch) = 0 */
                u.fir_live = true;
            }
        }
        if (ctx->d_sp_hist) {
            double *row = ctx->d_sp_hist + (size_t)ctx->sp_hist_cur * (size_t)ctx->nch * (size_t)ctx->sp_hist_len + (size_t)c * (size_t)ctx->sp_hist_len;
            if (r.sp_len) ps.add(blob + r.sp_off, row, (size_t)r.sp_len * sizeof(double));
            else ps.add(nullptr, row, (size_t)ctx->sp_hist_len * sizeof(double));       /* the source never spatialized: its history is zeros */
        }
        at += sizeof(r) + chain.size() * sizeof(StateSlot);
    }
    ps.append(extra);
    return ps.run(ctx);
}

/* check_only: everything a load checks before it touches the target, and nothing else */
static int load_common(gdg_ctx *ctx, const int *channels, int n, const void *blob, size_t bytes, bool device, const Pieces *extra = nullptr,
                       bool check_only = false) {
    if (!ctx || !blob) return GDG_ERR_INVALID;
    std::vector<int> chans;
    int rc = channel_list(ctx, channels, n, chans);
    if (rc != GDG_OK) return rc;
    if (device && ((uintptr_t)blob & 15)) return fail(ctx, GDG_ERR_INVALID, "state load: the device buffer must be 16-byte aligned");
    if (bytes < sizeof(StateHeader)) return fail(ctx, GDG_ERR_INVALID, "state load: %zu bytes are no blob (truncated)", bytes);
    enter(ctx, /*read_only=*/true);                   /* behind everything queued; what was made ahead stays until the blob is known to fit */
    StateHeader h;
    if (device) HIP_TRY(ctx, hipMemcpy(&h, blob, sizeof(h), hipMemcpyDeviceToHost));
    else memcpy(&h, blob, sizeof(h));
    if (memcmp(h.magic, GDG_STATE_MAGIC, 8) != 0) return fail(ctx, GDG_ERR_INVALID, "state load: not a state blob (bad magic)");
    if (h.version != GDG_STATE_VERSION)
        return fail(ctx, GDG_ERR_INVALID, "state load: format version %u, this library reads version %u", h.version, GDG_STATE_VERSION);
    if (h.total_bytes > bytes) return fail(ctx, GDG_ERR_INVALID, "state load: the blob is truncated (%zu of %llu bytes)", bytes, (unsigned long long)h.total_bytes);
    if (h.meta_bytes < sizeof(StateHeader) || h.meta_bytes > h.total_bytes || (h.meta_bytes & 15))
        return fail(ctx, GDG_ERR_INVALID, "state load: bad metadata size %u", h.meta_bytes);
    if (h.count != chans.size()) return fail(ctx, GDG_ERR_INVALID, "state load: the blob holds %u channel records, %zu channels given", h.count, chans.size());
    std::vector<unsigned char> meta(h.meta_bytes);
    if (device) HIP_TRY(ctx, hipMemcpy(meta.data(), blob, meta.size(), hipMemcpyDeviceToHost));
    else memcpy(meta.data(), blob, meta.size());
    rc = validate(ctx, chans, meta, h, check_only);
    if (rc != GDG_OK || check_only) return rc;
    if (device) {
        rc = apply(ctx, chans, static_cast<const unsigned char *>(blob), meta, extra);
    } else {
        unsigned char *stage = nullptr;
        HIP_TRY(ctx, ctx->arena.alloc((void **)&stage, h.total_bytes));
        hipError_t e = hipMemcpy(stage, blob, h.total_bytes, hipMemcpyHostToDevice);
        rc = e == hipSuccess ? apply(ctx, chans, stage, meta) : fail(ctx, GDG_ERR_HIP, "state load: %s", hipGetErrorString(e));
        hipStreamSynchronize(ctx->stream);
        ctx->arena.release(stage);
    }
    if (rc != GDG_OK) return rc;
    /* a context that never built a plan now holds state laid out at the blob's frame size and rate: a save before its first process
     * call records them (with frames = 0 that blob would say "every slot is fresh" beside slots that are not, and would not load) */
    if (h.frames > 0 && ctx->plan_frames == 0) { ctx->plan_frames = h.frames; ctx->plan_sr = h.rate; }
    drop_fir_ahead(ctx);
    ctx->premac_valid = false;
    ctx->dirty = true;
    return GDG_OK;
}

int gdg_state_load(gdg_ctx *ctx, const int *channels, int n, const void *blob, size_t bytes) {
    return load_common(ctx, channels, n, blob, bytes, false);
}
int gdg_state_load_device(gdg_ctx *ctx, const int *channels, int n, const void *d_blob, size_t bytes) {
    return load_common(ctx, channels, n, d_blob, bytes, true);
}

/* ---- for a checkpoint (api_checkpoint.cpp): all channels, a device buffer, the caller's pieces in the same launch ------------------------ */
int state_save_device_with(gdg_ctx *ctx, void *d_blob, size_t capacity, const Pieces *extra) {
    return save_common(ctx, nullptr, 0, d_blob, capacity, nullptr, true, extra);
}
int state_check_device(gdg_ctx *ctx, const void *d_blob, size_t bytes) {
    return load_common(ctx, nullptr, 0, d_blob, bytes, true, nullptr, true);
}
int state_load_device_with(gdg_ctx *ctx, const void *d_blob, size_t bytes, const Pieces *extra) {
    return load_common(ctx, nullptr, 0, d_blob, bytes, true, extra);
}
