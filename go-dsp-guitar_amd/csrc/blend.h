/*
 * blend.h -- the blend outputs (gdg_batch_set_blends, gdg_blend_rows; include/gdg.h states the arithmetic): a blend is a weighted sum of
 * chain output rows, s = w_0 x[c_0], then s = s + w_k x[c_k] in term order, every product and every add rounded on its own; a term may be
 * delayed by a whole number of samples (gdg_batch_set_blends_delayed) and pass a short FIR of its own (gdg_batch_set_blends_filtered).  The
 * three forms are ONE list with absent parts: here it is validated once (gdg_blend_check, gdg_blend_check_taps) and refused in one set of
 * words (gdg_blend_list_message, gdg_blend_taps_message), kept as one BlendSet, packed into one table (gdg_blend_pack) that is read through
 * one view (gdg_blend_view, gdg_blend_view_at) on the host and on the device, and summed on the host by one definition
 * (gdg_blend_sample_filtered).  Also here: the two rounded operations as __host__ __device__ inlines -- the kernels of blend_kernels.h use
 * them, and so can a stand-alone host program (tests/native/blend_check.cpp, blend_delay_check.cpp, blend_filter_check.cpp) --, and the
 * planner that turns alignment records into delays and signs (gdg_blend_delays_from_align); and, for the blend fit (include/gdg.h, FIT), the
 * validation of a list of fits, the table a launch reads, and the planner that turns fit records into weights (gdg_blend_weights_from_fit;
 * tests/native/fit_plan_check.cpp); and, for the Gram of a port list (include/gdg.h, GRAM), the validation of the list, the packed index
 * and the greedy planner that picks ports from Gram records (gdg_blend_pick_from_gram; tests/native/gram_plan_check.cpp); and, for the tap
 * fit (include/gdg.h, TAPFIT), the validation of its list, the table a launch reads and the planner that turns its records into taps
 * (gdg_blend_taps_from_tapfit; tests/native/tapfit_plan_check.cpp).  No HIP header is needed to compile this file.
 */
#ifndef GDG_BLEND_H
#define GDG_BLEND_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

/* the limits of include/gdg.h */
#ifndef GDG_BLEND_MAX_TERMS
#define GDG_BLEND_MAX_TERMS 32
#define GDG_BLEND_MAX_BLENDS 1024
#endif
#ifndef GDG_BLEND_MAX_DELAY
#define GDG_BLEND_MAX_DELAY 4096
#endif
#ifndef GDG_BLEND_MAX_TAPS
#define GDG_BLEND_MAX_TAPS 64
#endif

#if defined(__HIPCC__)
#define GDG_BLEND_HD __host__ __device__ __forceinline__
#else
#define GDG_BLEND_HD static inline
#endif

/* every product and every add is rounded before anything else sees it: never contracted into a fused multiply-add, on any compiler */
GDG_BLEND_HD double gdg_blend_mul(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dmul_rn(a, b);
#else
    volatile double r = a * b;
    return r;
#endif
}
GDG_BLEND_HD double gdg_blend_add(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dadd_rn(a, b);
#else
    volatile double r = a + b;
    return r;
#endif
}

/* ---- the configuration's arithmetic (host) --------------------------------------------------------------------------------------------- */
enum {
    BLEND_OK = 0,
    BLEND_COUNT = 1,                           /* n_blends outside 0 .. GDG_BLEND_MAX_BLENDS */
    BLEND_NULL = 2,                            /* a list is missing */
    BLEND_FIRST = 3,                           /* first[0] != 0, or first[b + 1] < first[b]: *blend = b */
    BLEND_EMPTY = 4,                           /* blend b has no term */
    BLEND_TERMS = 5,                           /* blend b has more than GDG_BLEND_MAX_TERMS terms */
    BLEND_CHANNEL = 6,                         /* term `term` of blend b names a channel outside [0, n_channels) */
    BLEND_WEIGHT = 7,                          /* ... has a weight that is not finite */
    BLEND_GAIN = 8,                            /* blend b's output gain is not finite */
    BLEND_DELAY = 9,                           /* term `term` of blend b has a delay outside 0 .. GDG_BLEND_MAX_DELAY */
    BLEND_TAP_FIRST = 10,                      /* tap_first does not start at 0, or descends at term `term` of blend b */
    BLEND_TAP_COUNT = 11,                      /* ... has more than GDG_BLEND_MAX_TAPS taps */
    BLEND_TAP = 12,                            /* ... has a tap that is not finite: *tap_at is its place among the term's taps */
    BLEND_REACH = 13                           /* ... reaches further back than GDG_BLEND_MAX_DELAY: d + max(T, 1) - 1 */
};

/* The whole list: n_blends blends, blend b's terms at [first[b], first[b + 1]) of channel[], weight[] and delay[]; delay: one per term, or
 * null (all 0); gain: one per blend, or null (all 1.0).  *blend, *term: the first offender (the term counted within its blend), -1 where the
 * status names none. */
static inline int gdg_blend_check(int n_blends, const int *first, const int *channel, const double *weight, const int *delay, const double *gain,
                                  int n_channels, int *blend, int *term) {
    *blend = *term = -1;
    if (n_blends < 0 || n_blends > GDG_BLEND_MAX_BLENDS) return BLEND_COUNT;
    if (n_blends == 0) return BLEND_OK;
    if (!first || !channel || !weight) return BLEND_NULL;
    if (first[0] != 0) { *blend = 0; return BLEND_FIRST; }
    for (int b = 0; b < n_blends; b++) {                                     /* the offsets first: nothing is read through a bad one */
        *blend = b;
        if (first[b + 1] < first[b]) return BLEND_FIRST;
        if (first[b + 1] == first[b]) return BLEND_EMPTY;
        if (first[b + 1] - first[b] > GDG_BLEND_MAX_TERMS) return BLEND_TERMS;
    }
    for (int b = 0; b < n_blends; b++) {
        *blend = b;
        for (int k = first[b]; k < first[b + 1]; k++) {
            *term = k - first[b];
            if (channel[k] < 0 || channel[k] >= n_channels) return BLEND_CHANNEL;
            if (!isfinite(weight[k])) return BLEND_WEIGHT;
            if (delay && (delay[k] < 0 || delay[k] > GDG_BLEND_MAX_DELAY)) return BLEND_DELAY;
        }
        *term = -1;
        if (gain && !isfinite(gain[b])) return BLEND_GAIN;
    }
    *blend = -1;
    return BLEND_OK;
}
/* the list without delays */
static inline int gdg_blend_check(int n_blends, const int *first, const int *channel, const double *weight, const double *gain, int n_channels,
                                  int *blend, int *term) {
    return gdg_blend_check(n_blends, first, channel, weight, (const int *)nullptr, gain, n_channels, blend, term);
}

/* The taps of a list that gdg_blend_check has passed (include/gdg.h, FILTERS): tap_first has one entry per term and one more, over all terms
 * of all blends; term k's taps are tap[tap_first[k] .. tap_first[k + 1]).  *blend, *term: the first offender, *tap_at: the tap where one is
 * named.  The offsets are checked first: nothing is read through a bad one. */
static inline int gdg_blend_check_taps(int n_blends, const int *first, const int *delay, const int *tap_first, const double *tap, int *blend, int *term, int *tap_at) {
    *blend = *term = *tap_at = -1;
    if (n_blends == 0 || !tap_first) return BLEND_OK;
    const int terms = first[n_blends];
    auto name = [&](int k) { int b = 0; while (first[b + 1] <= k) b++; *blend = b; *term = k - first[b]; };
    if (tap_first[0] != 0) { name(0); return BLEND_TAP_FIRST; }
    for (int k = 0; k < terms; k++) {
        if (tap_first[k + 1] < tap_first[k]) { name(k); return BLEND_TAP_FIRST; }
        if (tap_first[k + 1] - tap_first[k] > GDG_BLEND_MAX_TAPS) { name(k); return BLEND_TAP_COUNT; }
    }
    if (tap_first[terms] > 0 && !tap) return BLEND_NULL;
    for (int k = 0; k < terms; k++) {
        const int T = tap_first[k + 1] - tap_first[k], d = delay ? delay[k] : 0;
        for (int t = 0; t < T; t++) if (!isfinite(tap[tap_first[k] + t])) { name(k); *tap_at = t; return BLEND_TAP; }
        if (d + (T > 1 ? T : 1) - 1 > GDG_BLEND_MAX_DELAY) { name(k); return BLEND_REACH; }
    }
    return BLEND_OK;
}

/* what gdg_blend_check refused, in words, for the call `what`: one text for both callers.  standalone: the channels are the n_channels rows
 * of a stand-alone call ("blend rows"); otherwise the channels of a context ("set blends"), where 0 blends switch the outputs off */
static inline void gdg_blend_list_message(char *msg, size_t size, const char *what, bool standalone, int rc, int b, int k, int n_blends, const int *first, const int *channel,
                                          const double *weight, const int *delay, const double *gain, int n_channels) {
    const int at = b >= 0 && k >= 0 ? first[b] + k : 0;
    switch (rc) {
    case BLEND_COUNT: snprintf(msg, size, "%s: %d blends; 0 %sto %d", what, n_blends, standalone ? "" : "(off) ", GDG_BLEND_MAX_BLENDS); break;
    case BLEND_NULL: snprintf(msg, size, "%s: %d blends need first, channel and weight", what, n_blends); break;
    case BLEND_FIRST: snprintf(msg, size, "%s: blend %d: first[%d] = %d, first[%d] = %d; the offsets start at 0 and never descend", what, b, b, first[b], b + 1, first[b + 1]); break;
    case BLEND_EMPTY: snprintf(msg, size, "%s: blend %d has no term; 1 to %d", what, b, GDG_BLEND_MAX_TERMS); break;
    case BLEND_TERMS: snprintf(msg, size, "%s: blend %d has %d terms; 1 to %d", what, b, first[b + 1] - first[b], GDG_BLEND_MAX_TERMS); break;
    case BLEND_CHANNEL:
        if (standalone) snprintf(msg, size, "%s: blend %d, term %d names row %d of %d", what, b, k, channel[at], n_channels);
        else snprintf(msg, size, "%s: blend %d, term %d names channel %d, the context has channels 0 to %d", what, b, k, channel[at], n_channels - 1);
        break;
    case BLEND_WEIGHT: snprintf(msg, size, "%s: blend %d, term %d: weight = %g is not finite", what, b, k, weight[at]); break;
    case BLEND_DELAY: snprintf(msg, size, "%s: blend %d, term %d: delay = %d; 0 to %d%s", what, b, k, delay[at], GDG_BLEND_MAX_DELAY, standalone ? "" : " samples"); break;
    default: snprintf(msg, size, "%s: blend %d: gain = %g is not finite", what, b, gain[b]); break;
    }
}

/* what gdg_blend_check_taps refused, in words, for the call `what` ("set blends", "blend rows"): one text for both */
static inline void gdg_blend_taps_message(char *msg, size_t size, const char *what, int rc, int b, int k, int t, const int *first, const int *delay, const int *tap_first,
                                          const double *tap, int n_blends) {
    const int at = b >= 0 ? first[b] + k : 0, T = b >= 0 ? tap_first[at + 1] - tap_first[at] : 0, d = b >= 0 && delay ? delay[at] : 0;
    switch (rc) {
    case BLEND_NULL: snprintf(msg, size, "%s: tap_first names %d taps and tap is NULL", what, tap_first[first[n_blends]]); break;
    case BLEND_TAP_FIRST:
        snprintf(msg, size, "%s: blend %d, term %d: tap_first[%d] = %d, tap_first[%d] = %d; the offsets start at 0 and never descend", what, b, k, at, tap_first[at], at + 1, tap_first[at + 1]);
        break;
    case BLEND_TAP_COUNT: snprintf(msg, size, "%s: blend %d, term %d has %d taps; 0 to %d", what, b, k, T, GDG_BLEND_MAX_TAPS); break;
    case BLEND_TAP: snprintf(msg, size, "%s: blend %d, term %d: tap %d = %g is not finite", what, b, k, t, tap[tap_first[at] + t]); break;
    default:
        snprintf(msg, size, "%s: blend %d, term %d: a delay of %d samples and %d taps reach %d samples back; at most %d", what, b, k, d, T, d + (T > 1 ? T : 1) - 1, GDG_BLEND_MAX_DELAY);
        break;
    }
}

/* ---- the table a launch reads, and its view ------------------------------------------------------------------------------------------------ */
/* A checked list as the kernels take it, on the host or on the device.  A null member is an absent part: delay = every delay 0, tap_first and
 * tap = no term has a tap, gain = every gain 1.0. */
struct gdg_blend_view {
    int n_blends;
    const int *first, *channel;                /* n_blends + 1 offsets; one channel per term */
    const double *weight, *gain;               /* one per term; one per blend */
    const int *delay, *tap_first;              /* one per term; one per term and one more */
    const double *tap;
};

/* THE layout: first | channel | delay | tap_first | pad to 8 bytes | weight | gain | taps, an absent part taking no room; the doubles are
 * 8-byte aligned where base is.  The view of a table of n_blends blends and `terms` terms at base -- host bytes or their device copy; base
 * is never read here --, n_taps < 0: no tap_first and no taps.  *bytes (where asked for): the table's size. */
static inline gdg_blend_view gdg_blend_view_at(const void *base, int n_blends, int terms, bool delays, int n_taps, bool gains, size_t *bytes = nullptr) {
    gdg_blend_view v = { n_blends, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
    uintptr_t at = (uintptr_t)base;
    auto take = [&](size_t count, size_t size, bool there) { const uintptr_t p = there ? at : 0; if (there) at += count * size; return p; };
    if (n_blends > 0) {
        v.first = (const int *)take((size_t)n_blends + 1, sizeof(int), true);
        v.channel = (const int *)take((size_t)terms, sizeof(int), true);
        v.delay = (const int *)take((size_t)terms, sizeof(int), delays);
        v.tap_first = (const int *)take((size_t)terms + 1, sizeof(int), n_taps >= 0);
        at += (8 - (at - (uintptr_t)base) % 8) % 8;
        v.weight = (const double *)take((size_t)terms, sizeof(double), true);
        v.gain = (const double *)take((size_t)n_blends, sizeof(double), gains);
        v.tap = (const double *)take((size_t)(n_taps > 0 ? n_taps : 0), sizeof(double), n_taps >= 0);
    }
    if (bytes) *bytes = (size_t)(at - (uintptr_t)base);
    return v;
}

/* a checked list as the table's bytes; delay, tap_first (with tap) and gain may be null: absent */
static inline std::vector<unsigned char> gdg_blend_pack(int n_blends, const int *first, const int *channel, const double *weight, const double *gain, const int *delay,
                                                        const int *tap_first, const double *tap) {
    std::vector<unsigned char> packed;
    if (n_blends <= 0) return packed;
    const int terms = first[n_blends], n_taps = tap_first ? tap_first[terms] : -1;
    size_t bytes = 0;
    gdg_blend_view_at(nullptr, n_blends, terms, delay != nullptr, n_taps, gain != nullptr, &bytes);
    packed.assign(bytes, 0);
    const gdg_blend_view v = gdg_blend_view_at(packed.data(), n_blends, terms, delay != nullptr, n_taps, gain != nullptr);
    auto put = [](const void *to, const void *from, size_t n) { if (n) memcpy(const_cast<void *>(to), from, n); };
    put(v.first, first, ((size_t)n_blends + 1) * sizeof(int));
    put(v.channel, channel, (size_t)terms * sizeof(int));
    put(v.weight, weight, (size_t)terms * sizeof(double));
    if (delay) put(v.delay, delay, (size_t)terms * sizeof(int));
    if (gain) put(v.gain, gain, (size_t)n_blends * sizeof(double));
    if (tap_first) put(v.tap_first, tap_first, ((size_t)terms + 1) * sizeof(int));
    if (n_taps > 0) put(v.tap, tap, (size_t)n_taps * sizeof(double));
    return packed;
}

/* the list in force */
struct BlendSet {
    std::vector<int> first, channel;           /* first: count() + 1 offsets, empty = off */
    std::vector<double> weight, gain;          /* gain: one per blend, 1.0 where none was given */
    std::vector<int> delay;                    /* one per term; empty = every delay 0, and the list is what it was before delays existed */
    int count() const { return first.empty() ? 0 : (int)first.size() - 1; }
    int terms() const { return (int)channel.size(); }
    /* the taps (FILTERS): terms() + 1 offsets into tap; both empty = no term has a tap, and the list is what it was before taps existed */
    std::vector<int> tap_first;
    std::vector<double> tap;
    int max_delay() const { int m = 0; for (int d : delay) if (d > m) m = d; return m; }
    int taps(int k) const { return tap_first.empty() ? 0 : tap_first[(size_t)k + 1] - tap_first[(size_t)k]; }
    /* how far back a term reads: the largest d_k + max(T_k, 1) - 1; without taps the largest delay */
    int max_reach() const {
        int m = max_delay();
        for (int k = 0; k < terms() && !tap_first.empty(); k++) { const int r = delay[(size_t)k] + (taps(k) > 1 ? taps(k) : 1) - 1; if (r > m) m = r; }
        return m;
    }
    bool unit_gains() const { for (double g : gain) if (g != 1.0) return false; return true; }
    /* the table as a launch reads it (gdg_blend_pack), made when the list is taken: the delays are there only while one of them is not 0 or a
     * term has taps, tap_first and the taps only while a term has taps, the gains always */
    std::vector<unsigned char> packed;
    void pack() {
        packed = gdg_blend_pack(count(), first.data(), channel.data(), weight.data(), gain.data(), delay.empty() ? nullptr : delay.data(),
                                tap_first.empty() ? nullptr : tap_first.data(), tap.data());
    }
    /* the view of `packed` or of a copy of it at base */
    gdg_blend_view view(const void *base) const { return gdg_blend_view_at(base, count(), terms(), !delay.empty(), tap_first.empty() ? -1 : (int)tap.size(), true); }
    /* where the doubles and where the taps begin: the view of a table at address 0 holds offsets */
    size_t packed_ints() const { return (size_t)(uintptr_t)view(nullptr).weight; }
    size_t packed_taps() const { return packed_ints() + (weight.size() + gain.size()) * sizeof(double); }
};

/* whole or not at all: a refused list leaves the one in force as it is */
static inline int gdg_blend_replace(BlendSet &set, int n_blends, const int *first, const int *channel, const double *weight, const int *delay,
                                    const int *tap_first, const double *tap, const double *gain, int n_channels, int *blend, int *term) {
    int rc = gdg_blend_check(n_blends, first, channel, weight, delay, gain, n_channels, blend, term), tap_at = -1;
    if (rc == BLEND_OK) rc = gdg_blend_check_taps(n_blends, first, delay, tap_first, tap, blend, term, &tap_at);
    if (rc != BLEND_OK) return rc;
    BlendSet next;
    if (n_blends > 0) {
        const int terms = first[n_blends];
        next.first.assign(first, first + n_blends + 1);
        next.channel.assign(channel, channel + terms);
        next.weight.assign(weight, weight + terms);
        if (gain) next.gain.assign(gain, gain + n_blends);
        else next.gain.assign((size_t)n_blends, 1.0);
        if (delay) {
            next.delay.assign(delay, delay + terms);
            if (next.max_delay() == 0) next.delay.clear();                   /* all zeros: the list without delays */
        }
        if (tap_first && tap_first[terms] > 0) {                             /* no tap anywhere: the list without taps */
            next.tap_first.assign(tap_first, tap_first + terms + 1);
            next.tap.assign(tap, tap + tap_first[terms]);
            if (next.delay.empty()) next.delay.assign((size_t)terms, 0);     /* a filtered table always carries its delays */
        }
    }
    next.pack();
    set = next;
    return BLEND_OK;
}
static inline int gdg_blend_replace(BlendSet &set, int n_blends, const int *first, const int *channel, const double *weight, const int *delay,
                                    const double *gain, int n_channels, int *blend, int *term) {
    return gdg_blend_replace(set, n_blends, first, channel, weight, delay, (const int *)nullptr, (const double *)nullptr, gain, n_channels, blend, term);
}
static inline int gdg_blend_replace(BlendSet &set, int n_blends, const int *first, const int *channel, const double *weight, const double *gain,
                                    int n_channels, int *blend, int *term) {
    return gdg_blend_replace(set, n_blends, first, channel, weight, (const int *)nullptr, gain, n_channels, blend, term);
}

/* ---- the sum on the host: ONE definition (include/gdg.h, BLEND, DELAYS, FILTERS) --------------------------------------------------------------- */
/* sample i - d of a row; what lies in front of its sample 0 is `history` -- GDG_BLEND_MAX_DELAY doubles, the last of them sample -1 -- or,
 * without one, +0.0 */
static inline double gdg_blend_delayed_x(const double *row, const double *history, size_t i, int d) {
    if (i >= (size_t)d) return row[i - (size_t)d];
    return history ? history[(size_t)GDG_BLEND_MAX_DELAY + i - (size_t)d] : 0.0;
}

/* sample i of the blend with terms [k0, k1): x_k[i] = x[c_k][i - d_k], or through its taps h_k[0] x[c_k][i - d_k], then + h_k[t] x[c_k][i -
 * d_k - t] in ascending t.  history = one run per row, or null; delay = one per term, or null (all 0); tap_first = one offset per term and
 * one more, or null (no taps).  A term with T == 0 is the delayed sample, and with d == 0 the row's own: the bits of the sums without */
static inline double gdg_blend_sample_filtered(const double *const *rows, const double *const *history, size_t i, const int *channel, const double *weight,
                                               const int *delay, const int *tap_first, const double *tap, int k0, int k1) {
    auto x = [&](int k) {
        const double *row = rows[channel[k]], *hist = history ? history[channel[k]] : nullptr;
        const int d = delay ? delay[k] : 0, T = tap_first ? tap_first[k + 1] - tap_first[k] : 0;
        if (T == 0) return gdg_blend_delayed_x(row, hist, i, d);
        const double *h = tap + tap_first[k];
        double f = gdg_blend_mul(h[0], gdg_blend_delayed_x(row, hist, i, d));
        for (int t = 1; t < T; t++) f = gdg_blend_add(f, gdg_blend_mul(h[t], gdg_blend_delayed_x(row, hist, i, d + t)));
        return f;
    };
    double s = gdg_blend_mul(weight[k0], x(k0));
    for (int k = k0 + 1; k < k1; k++) s = gdg_blend_add(s, gdg_blend_mul(weight[k], x(k)));
    return s;
}

/* a checked list over `samples` samples of every row: out[b][i] */
static inline void gdg_blend_sum_host_filtered(const double *const *rows, const double *const *history, size_t samples, int n_blends, const int *first,
                                               const int *channel, const double *weight, const int *delay, const int *tap_first, const double *tap,
                                               double *const *out) {
    for (int b = 0; b < n_blends; b++)
        for (size_t i = 0; i < samples; i++)
            out[b][i] = gdg_blend_sample_filtered(rows, history, i, channel, weight, delay, tap_first, tap, first[b], first[b + 1]);
}

/* the names of the list without taps, and without delays as well */
static inline double gdg_blend_sample_delayed(const double *const *rows, const double *const *history, size_t i, const int *channel, const double *weight,
                                              const int *delay, int k0, int k1) {
    return gdg_blend_sample_filtered(rows, history, i, channel, weight, delay, nullptr, nullptr, k0, k1);
}
static inline void gdg_blend_sum_host_delayed(const double *const *rows, const double *const *history, size_t samples, int n_blends, const int *first,
                                              const int *channel, const double *weight, const int *delay, double *const *out) {
    gdg_blend_sum_host_filtered(rows, history, samples, n_blends, first, channel, weight, delay, nullptr, nullptr, out);
}
static inline double gdg_blend_sample(const double *const *rows, size_t i, const int *channel, const double *weight, int k0, int k1) {
    return gdg_blend_sample_filtered(rows, nullptr, i, channel, weight, nullptr, nullptr, nullptr, k0, k1);
}
static inline void gdg_blend_sum_host(const double *const *rows, size_t samples, int n_blends, const int *first, const int *channel, const double *weight,
                                      double *const *out) {
    gdg_blend_sum_host_filtered(rows, nullptr, samples, n_blends, first, channel, weight, nullptr, nullptr, nullptr, out);
}

/* ---- the taps of a fractional delay (gdg_blend_fraction_taps) ---------------------------------------------------------------------------- */
/* T taps (even, 2 .. GDG_BLEND_MAX_TAPS) that delay by T/2 - 1 + f samples, 0 <= f < 1: sinc(u) (0.5 + 0.5 cos(2 pi u / T)) with u = t -
 * (T/2 - 1) - f, divided by their sum (added in ascending t).  f == 0: the unit impulse at T/2 - 1, exactly, and no call into libm.
 * false: an argument out of range; nothing is written. */
static inline bool gdg_blend_fraction_taps_plan(int T, double f, double *tap) {
    if (T < 2 || T > GDG_BLEND_MAX_TAPS || (T & 1) || !(f >= 0.0 && f < 1.0) || !tap) return false;
    if (f == 0.0) {
        for (int t = 0; t < T; t++) tap[t] = t == T / 2 - 1 ? 1.0 : 0.0;
        return true;
    }
    const double pi = 3.141592653589793;
    double h[GDG_BLEND_MAX_TAPS], sum = 0.0;
    for (int t = 0; t < T; t++) {
        const double u = (double)(t - (T / 2 - 1)) - f;                      /* never 0: 0 < f < 1 */
        h[t] = sin(pi * u) / (pi * u) * (0.5 + 0.5 * cos(2.0 * pi * u / (double)T));
        sum += h[t];
    }
    for (int t = 0; t < T; t++) tap[t] = h[t] / sum;
    return true;
}

/* ---- the delays from the alignment records (gdg_blend_delays_from_align) --------------------------------------------------------------- */
struct gdg_blend_align_rec { double corr, corr0, ref_sq, sq_at_lag; int32_t lag; uint32_t reserved; };      /* gdg_block_align of include/gdg.h */

enum {
    BLEND_PLAN_OK = 0,
    BLEND_PLAN_ARGS = 1,                       /* a list is missing, a count is out of range, min_coeff lies outside [0, 1] */
    BLEND_PLAN_LIST = 2,                       /* the CSR form of *blend is broken, it names a port outside [0, ports), or that port's reference is none */
    BLEND_PLAN_MIXED = 3                       /* the terms of *blend do not share one reference port */
};

/* lag and sign of one port from its records: the blocks with both energies and a coefficient of at least min_coeff count; the lower median
 * of their lags, the sign of the sum of their corr; no such block: lag 0, sign +1 */
static inline void gdg_blend_port_lag(const gdg_blend_align_rec *rec, size_t blocks, double min_coeff, int *lag, int *sign) {
    std::vector<int> lags;
    double sum = 0.0;
    for (size_t b = 0; b < blocks; b++) {
        const gdg_blend_align_rec &r = rec[b];
        if (!(r.ref_sq > 0.0) || !(r.sq_at_lag > 0.0)) continue;
        if (!(fabs(r.corr) / sqrt(r.ref_sq * r.sq_at_lag) >= min_coeff)) continue;
        lags.push_back(r.lag);
        sum += r.corr;
    }
    *lag = 0;
    *sign = 1;
    if (lags.empty()) return;
    for (size_t i = 1; i < lags.size(); i++) {                               /* sorted by insertion: no <algorithm> for a few blocks */
        const int v = lags[i];
        size_t j = i;
        for (; j > 0 && lags[j - 1] > v; j--) lags[j] = lags[j - 1];
        lags[j] = v;
    }
    *lag = lags[(lags.size() - 1) / 2];
    *sign = sum < 0.0 ? -1 : 1;
}

/* records[ports][blocks] as measured against ref[ports]; the blends in CSR form with `channel` naming a port.  Everything is checked before
 * delay[] and sign[] (one per term) are written; *blend: the offender. */
static inline int gdg_blend_plan_delays(const gdg_blend_align_rec *records, int ports, size_t blocks, const int *ref, double min_coeff, int n_blends,
                                        const int *first, const int *channel, int *delay, int *sign, int *blend) {
    *blend = -1;
    if (ports < 1 || n_blends < 0 || n_blends > GDG_BLEND_MAX_BLENDS || !ref || (blocks && !records) || !(min_coeff >= 0.0 && min_coeff <= 1.0)) return BLEND_PLAN_ARGS;
    if (n_blends == 0) return BLEND_PLAN_OK;
    if (!first || !channel || !delay || !sign) return BLEND_PLAN_ARGS;
    if (first[0] != 0) { *blend = 0; return BLEND_PLAN_LIST; }
    for (int b = 0; b < n_blends; b++) {
        *blend = b;
        if (first[b + 1] <= first[b] || first[b + 1] - first[b] > GDG_BLEND_MAX_TERMS) return BLEND_PLAN_LIST;
    }
    std::vector<int> root((size_t)n_blends, -1);
    for (int b = 0; b < n_blends; b++) {
        *blend = b;
        int r = -1;
        for (int k = first[b]; k < first[b + 1]; k++) {                      /* the terms that are measured against another port: all against one */
            const int c = channel[k];
            if (c < 0 || c >= ports || ref[c] < -1 || ref[c] >= ports) return BLEND_PLAN_LIST;
            if (ref[c] < 0 || ref[c] == c) continue;
            if (r >= 0 && r != ref[c]) return BLEND_PLAN_MIXED;
            r = ref[c];
        }
        for (int k = first[b]; k < first[b + 1]; k++) {                      /* a term measured against nothing else has to BE that port */
            const int c = channel[k];
            if (ref[c] >= 0 && ref[c] != c) continue;
            if (r >= 0 && r != c) return BLEND_PLAN_MIXED;
            r = c;
        }
        root[(size_t)b] = r;
    }
    *blend = -1;
    for (int b = 0; b < n_blends; b++) {
        int lag[GDG_BLEND_MAX_TERMS], most = 0;
        for (int k = first[b]; k < first[b + 1]; k++) {
            const int c = channel[k], t = k - first[b];
            lag[t] = 0;
            sign[k] = 1;
            if (c != root[(size_t)b]) gdg_blend_port_lag(records + (size_t)c * blocks, blocks, min_coeff, &lag[t], &sign[k]);
            if (t == 0 || lag[t] > most) most = lag[t];
        }
        for (int k = first[b]; k < first[b + 1]; k++) delay[k] = most - lag[k - first[b]];
    }
    return BLEND_PLAN_OK;
}

/* ---- the blend fit (include/gdg.h, FIT): a list of fits, and the weights from their records (gdg_blend_weights_from_fit) ---------------- */
#ifndef GDG_FIT_MAX_TERMS
#define GDG_FIT_MAX_TERMS 8
#define GDG_FIT_MAX_FITS 256
#endif
#define GDG_FIT_TABLE_INTS (2 + GDG_FIT_MAX_TERMS)                           /* a fit as the kernel reads it: target | terms | port[8] */

enum {
    FIT_OK = 0,
    FIT_COUNT = 1,                             /* n_fits outside 0 .. GDG_FIT_MAX_FITS */
    FIT_NULL = 2,                              /* a list is missing */
    FIT_FIRST = 3,                             /* first[0] != 0, or first[f + 1] < first[f]: *fit = f */
    FIT_TERMS = 4,                             /* fit f has no term or more than GDG_FIT_MAX_TERMS */
    FIT_PORT = 5,                              /* term `term` of fit f names a port outside [0, n_ports) */
    FIT_TARGET = 6                             /* fit f's target lies outside [0, n_ports) */
};

/* The list in its CSR form: fit f has the terms port[first[f] .. first[f + 1]) and the target target[f].  n_ports < 0: the port count is
 * not known yet (it is the job's: N + 3 + B) and only negative ports are refused.  *fit, *term: the first offender, -1 where none is named. */
static inline int gdg_fit_check(int n_fits, const int *first, const int *port, const int *target, int n_ports, int *fit, int *term) {
    *fit = *term = -1;
    if (n_fits < 0 || n_fits > GDG_FIT_MAX_FITS) return FIT_COUNT;
    if (n_fits == 0) return FIT_OK;
    if (!first || !port || !target) return FIT_NULL;
    if (first[0] != 0) { *fit = 0; return FIT_FIRST; }
    for (int f = 0; f < n_fits; f++) {                                       /* the offsets first: nothing is read through a bad one */
        *fit = f;
        if (first[f + 1] < first[f]) return FIT_FIRST;
        if (first[f + 1] == first[f] || first[f + 1] - first[f] > GDG_FIT_MAX_TERMS) return FIT_TERMS;
    }
    for (int f = 0; f < n_fits; f++) {
        *fit = f;
        if (target[f] < 0 || (n_ports >= 0 && target[f] >= n_ports)) return FIT_TARGET;
        for (int k = first[f]; k < first[f + 1]; k++)
            if (port[k] < 0 || (n_ports >= 0 && port[k] >= n_ports)) { *term = k - first[f]; return FIT_PORT; }
    }
    *fit = -1;
    return FIT_OK;
}

/* the list in force, as the table a launch reads: [fits][target | terms | port[8]], the ports behind a fit's last term 0 */
struct FitSet {
    std::vector<int> table;
    int count() const { return (int)(table.size() / GDG_FIT_TABLE_INTS); }
    int target(int f) const { return table[(size_t)f * GDG_FIT_TABLE_INTS]; }
    int terms(int f) const { return table[(size_t)f * GDG_FIT_TABLE_INTS + 1]; }
    int port(int f, int k) const { return table[(size_t)f * GDG_FIT_TABLE_INTS + 2 + (size_t)k]; }
    /* the first fit that names a port outside [0, n_ports): -1 = none; *term: the term, -1 = the target */
    int first_outside(int n_ports, int *term) const {
        for (int f = 0; f < count(); f++) {
            *term = -1;
            if (target(f) >= n_ports) return f;
            for (int k = 0; k < terms(f); k++) if (port(f, k) >= n_ports) { *term = k; return f; }
        }
        return -1;
    }
};

/* a checked list as a table */
static inline std::vector<int> gdg_fit_table(int n_fits, const int *first, const int *port, const int *target) {
    std::vector<int> t((size_t)n_fits * GDG_FIT_TABLE_INTS, 0);
    for (int f = 0; f < n_fits; f++) {
        int *e = &t[(size_t)f * GDG_FIT_TABLE_INTS];
        e[0] = target[f];
        e[1] = first[f + 1] - first[f];
        for (int k = first[f]; k < first[f + 1]; k++) e[2 + k - first[f]] = port[k];
    }
    return t;
}

struct gdg_blend_fit_rec { double tt, tx[GDG_FIT_MAX_TERMS], xx[GDG_FIT_MAX_TERMS * (GDG_FIT_MAX_TERMS + 1) / 2]; uint32_t skipped, terms; };      /* gdg_block_fit of include/gdg.h */

enum {
    FIT_PLAN_OK = 0,
    FIT_PLAN_ARGS = 1,                         /* a list is missing, a count is out of range, no block, ridge is negative or not finite */
    FIT_PLAN_TERMS = 2,                        /* the records of *fit do not agree on a term count in 1 .. GDG_FIT_MAX_TERMS */
    FIT_PLAN_PIVOT = 3                         /* the factorisation of *fit met a pivot at or below the bound: a silent term, or a port twice without a ridge */
};

/* The ONE solve at any size, for a fit's sums, a pick's (gdg_blend_pick) and a tap fit's (gdg_blend_plan_taps): T, b[K] and the lower triangle
 * of G[K][K] (row j at G + j * ld) in -> (G + ridge * mean(diag G) I) w = b by an unpivoted Cholesky factorisation in row order, *res = max(0,
 * T - 2 w.b + w'Gw) / T (0 where T == 0).  false: a pivot at or below K * 2^-52 * max(diag G) in row *pivot; w and *res are then not to be
 * used.  The upper triangle of G is filled here.  Lo: K * ld doubles of room, y: K. */
static inline bool gdg_solve_n(int K, double T, const double *b, double *G, size_t ld, double ridge, double *w, double *res, int *pivot, double *Lo, double *y) {
    for (int j = 0; j < K; j++) for (int k = j + 1; k < K; k++) G[j * ld + k] = G[k * ld + j];
    double trace = 0.0, most = 0.0;
    for (int j = 0; j < K; j++) { trace += G[j * ld + j]; if (G[j * ld + j] > most) most = G[j * ld + j]; }
    const double shift = ridge * (trace / (double)K), least = (double)K * 2.220446049250313e-16 * most;      /* K * 2^-52 * max(diag G) */
    for (int j = 0; j < K; j++) {
        double d = G[j * ld + j] + shift;
        for (int k = 0; k < j; k++) d -= Lo[j * ld + k] * Lo[j * ld + k];
        if (!(d > least)) { *pivot = j; return false; }
        Lo[j * ld + j] = sqrt(d);
        for (int i = j + 1; i < K; i++) {
            double s = G[i * ld + j];
            for (int k = 0; k < j; k++) s -= Lo[i * ld + k] * Lo[j * ld + k];
            Lo[i * ld + j] = s / Lo[j * ld + j];
        }
    }
    for (int j = 0; j < K; j++) {                                        /* L y = b, then L' w = y */
        double s = b[j];
        for (int k = 0; k < j; k++) s -= Lo[j * ld + k] * y[k];
        y[j] = s / Lo[j * ld + j];
    }
    for (int j = K - 1; j >= 0; j--) {
        double s = y[j];
        for (int k = j + 1; k < K; k++) s -= Lo[k * ld + j] * w[k];
        w[j] = s / Lo[j * ld + j];
    }
    double wb = 0.0, wGw = 0.0;
    for (int j = 0; j < K; j++) {
        wb += w[j] * b[j];
        double row = 0.0;
        for (int k = 0; k < K; k++) row += G[j * ld + k] * w[k];
        wGw += w[j] * row;
    }
    const double left = T - 2.0 * wb + wGw;
    *res = T == 0.0 ? 0.0 : (left > 0.0 ? left : 0.0) / T;
    return true;
}

/* ... at the fits' and the picks' size: up to 8 rows on the stack */
static inline bool gdg_fit_solve(int K, double T, const double *b, double (*G)[GDG_FIT_MAX_TERMS], double ridge, double *w, double *res) {
    constexpr int M = GDG_FIT_MAX_TERMS;
    double Lo[M][M], y[M];
    int pivot = -1;
    return gdg_solve_n(K, T, b, &G[0][0], (size_t)M, ridge, w, res, &pivot, &Lo[0][0], y);
}

/* records[n_fits][blocks].  Per fit: the blocks' sums added in block order -- T, b[K], G[K][K] --, (G + ridge * mean(diag G) * I) w = b by
 * an unpivoted Cholesky factorisation in term order, residual = max(0, T - 2 w.b + w'Gw) / T (0 where T == 0).  Every fit is solved before
 * weight[n_fits][8] and residual[n_fits] are written; *fit: the offender. */
static inline int gdg_blend_plan_weights(const gdg_blend_fit_rec *records, int n_fits, size_t blocks, double ridge, double *weight, double *residual, int *fit) {
    *fit = -1;
    if (n_fits < 0 || n_fits > GDG_FIT_MAX_FITS || !(ridge >= 0.0) || !isfinite(ridge)) return FIT_PLAN_ARGS;
    if (n_fits == 0) return FIT_PLAN_OK;
    if (!records || !weight || !residual || blocks == 0) return FIT_PLAN_ARGS;
    constexpr int M = GDG_FIT_MAX_TERMS;
    std::vector<double> w_all((size_t)n_fits * M, 0.0), res_all((size_t)n_fits, 0.0);
    for (int f = 0; f < n_fits; f++) {
        *fit = f;
        const gdg_blend_fit_rec *rec = records + (size_t)f * blocks;
        const int K = (int)rec[0].terms;
        if (K < 1 || K > M) return FIT_PLAN_TERMS;
        double T = 0.0, b[M], G[M][M];
        for (int j = 0; j < K; j++) { b[j] = 0.0; for (int k = 0; k < K; k++) G[j][k] = 0.0; }
        for (size_t q = 0; q < blocks; q++) {
            if ((int)rec[q].terms != K) return FIT_PLAN_TERMS;
            T += rec[q].tt;
            for (int j = 0; j < K; j++) {
                b[j] += rec[q].tx[j];
                for (int k = 0; k <= j; k++) G[j][k] += rec[q].xx[j * (j + 1) / 2 + k];
            }
        }
        if (!gdg_fit_solve(K, T, b, G, ridge, &w_all[(size_t)f * M], &res_all[(size_t)f])) return FIT_PLAN_PIVOT;
    }
    *fit = -1;
    memcpy(weight, w_all.data(), w_all.size() * sizeof(double));
    memcpy(residual, res_all.data(), res_all.size() * sizeof(double));
    return FIT_PLAN_OK;
}

/* ---- the fraction of a delay from fit records (gdg_blend_fractions_from_fit) ---------------------------------------------------------------- */
enum {
    FRACTION_OK = 0,
    FRACTION_ARGS = 1,                         /* a list is missing, a count is out of range, no block, steps outside 1 .. 4 */
    FRACTION_TERMS = 2,                        /* a record of *fit has another term count than 2 steps - 1 */
    FRACTION_NONFINITE = 3                     /* a sum of *fit -- tt, a tx or a diagonal xx -- is a NaN or inf */
};

/* records[n_fits][blocks]; a fit has the 2Q - 1 candidates of one channel, term k at (k - (Q - 1)) / Q samples, measured against the target.
 * The blocks' sums are added in block order; the candidate with the largest tx[k] / sqrt(xx[k][k]) among those with xx[k][k] > 0 wins, the
 * earlier entry on a tie; step[f] = k - (Q - 1), 0 where tt <= 0 or no candidate is admissible.  Every fit is decided before step[] is
 * written; *fit: the offender. */
static inline int gdg_blend_plan_fractions(const gdg_blend_fit_rec *records, int n_fits, size_t blocks, int steps, int *step, int *fit) {
    *fit = -1;
    if (n_fits < 0 || n_fits > GDG_FIT_MAX_FITS || steps < 1 || steps > 4) return FRACTION_ARGS;
    if (n_fits == 0) return FRACTION_OK;
    if (!records || !step || blocks == 0) return FRACTION_ARGS;
    const int K = 2 * steps - 1;
    std::vector<int> all((size_t)n_fits, 0);
    for (int f = 0; f < n_fits; f++) {
        *fit = f;
        const gdg_blend_fit_rec *rec = records + (size_t)f * blocks;
        double tt = 0.0, tx[GDG_FIT_MAX_TERMS], xx[GDG_FIT_MAX_TERMS];
        for (int k = 0; k < K; k++) tx[k] = xx[k] = 0.0;
        for (size_t q = 0; q < blocks; q++) {
            if ((int)rec[q].terms != K) return FRACTION_TERMS;
            tt += rec[q].tt;
            for (int k = 0; k < K; k++) { tx[k] += rec[q].tx[k]; xx[k] += rec[q].xx[k * (k + 1) / 2 + k]; }
        }
        if (!isfinite(tt)) return FRACTION_NONFINITE;
        for (int k = 0; k < K; k++) if (!isfinite(tx[k]) || !isfinite(xx[k])) return FRACTION_NONFINITE;
        if (!(tt > 0.0)) continue;
        int best = -1;
        double best_score = 0.0;
        for (int k = 0; k < K; k++) {
            if (!(xx[k] > 0.0)) continue;
            const double score = tx[k] / sqrt(xx[k]);
            if (best < 0 || score > best_score) { best = k; best_score = score; }
        }
        if (best >= 0) all[(size_t)f] = best - (steps - 1);
    }
    *fit = -1;
    memcpy(step, all.data(), all.size() * sizeof(int));
    return FRACTION_OK;
}

/* ---- the Gram of a port list (include/gdg.h, GRAM): the list, the packed index, and the picks from its records (gdg_blend_pick_from_gram) ---- */
#ifndef GDG_GRAM_MAX_PORTS
#define GDG_GRAM_MAX_PORTS 512
#endif

/* entry (i, j), j <= i, of a record: the lower triangle by rows -- the fit's xx layout */
static inline size_t gdg_gram_index(size_t i, size_t j) { return i * (i + 1) / 2 + j; }
static inline size_t gdg_gram_doubles(size_t n_ports) { return n_ports * (n_ports + 1) / 2; }

/* the first entry of a list outside [0, n_rows) -- n_rows < 0: the count is not known yet (the job's N + 3 + B), only negatives --, -1 = none */
static inline int gdg_gram_list_bad(const int *port, int n_ports, int n_rows) {
    for (int i = 0; i < n_ports; i++) if (port[i] < 0 || (n_rows >= 0 && port[i] >= n_rows)) return i;
    return -1;
}

/* the first entry that repeats an earlier one, -1 = none; *earlier: that one's position */
static inline int gdg_gram_list_repeat(const int *port, int n_ports, int *earlier) {
    for (int i = 1; i < n_ports; i++)
        for (int j = 0; j < i; j++) if (port[j] == port[i]) { *earlier = j; return i; }
    return -1;
}

enum {
    PICK_OK = 0,
    PICK_ARGS = 1,                             /* a list is missing, a count is out of range, no block, ridge or min_gain negative or not finite */
    PICK_POSITION = 2,                         /* the target or candidate *at lies outside the list (*at = -1: the target) */
    PICK_REPEAT = 3,                           /* candidate *at repeats an earlier one or is the target */
    PICK_NONFINITE = 4,                        /* the summed Gram has a NaN or inf in the row or column of list position *at */
    PICK_SILENT = 5                            /* T = G[target][target] <= 0 */
};

/* records[blocks][n_ports (n_ports + 1) / 2]; target and candidate[] are positions in the list.  The blocks' records are added in block
 * order with plain adds; T = G[target][target].  Greedy forward selection: with the set S picked so far, in pick order, every candidate not
 * in S is tried in list order -- gdg_fit_solve on S and the candidate, whose unpivoted factorisation extends the one of S by the candidate's
 * row; a candidate that brings a pivot at or below the bound is skipped: a silent port, or a duplicate of a picked one --, the smallest
 * residual share wins, the earlier entry on a tie.  It stops after max_terms picks, when the best candidate improves the share by less than
 * min_gain (the share before the first pick is 1), or when no candidate is admissible.  Everything is decided before picked[8], weight[8],
 * residual[8] and *n_picked are written; entries behind *n_picked are -1, 0.0 and 0.0.  The weights are those of gdg_fit_solve for the picked
 * ports in pick order: bit for bit gdg_blend_plan_weights on a fit record with the same sums. */
static inline int gdg_blend_pick(const double *records, int n_ports, size_t blocks, int target, const int *candidate, int n_candidates, int max_terms, double ridge,
                                 double min_gain, int *picked, double *weight, double *residual, int *n_picked, int *at) {
    *at = -1;
    constexpr int M = GDG_FIT_MAX_TERMS;
    if (n_ports < 2 || n_ports > GDG_GRAM_MAX_PORTS || blocks == 0 || n_candidates < 1 || n_candidates >= n_ports || max_terms < 1 || max_terms > M ||
        !(ridge >= 0.0) || !isfinite(ridge) || !(min_gain >= 0.0) || !isfinite(min_gain) || !records || !candidate || !picked || !weight || !residual || !n_picked)
        return PICK_ARGS;
    if (target < 0 || target >= n_ports) return PICK_POSITION;
    for (int c = 0; c < n_candidates; c++) {
        *at = c;
        if (candidate[c] < 0 || candidate[c] >= n_ports) return PICK_POSITION;
        if (candidate[c] == target) return PICK_REPEAT;
        for (int d = 0; d < c; d++) if (candidate[d] == candidate[c]) return PICK_REPEAT;
    }
    const size_t E = gdg_gram_doubles((size_t)n_ports);
    std::vector<double> sum(E, 0.0);
    for (size_t q = 0; q < blocks; q++) for (size_t e = 0; e < E; e++) sum[e] += records[q * E + e];
    auto g = [&](int i, int j) { return i >= j ? sum[gdg_gram_index((size_t)i, (size_t)j)] : sum[gdg_gram_index((size_t)j, (size_t)i)]; };
    /* what the picks can read: the entries among the target and the candidates */
    for (int a = -1; a < n_candidates; a++) {
        const int i = a < 0 ? target : candidate[a];
        *at = i;
        if (!isfinite(g(i, target))) return PICK_NONFINITE;
        for (int c = 0; c < n_candidates; c++) if (!isfinite(g(i, candidate[c]))) return PICK_NONFINITE;
    }
    *at = -1;
    const double T = g(target, target);
    if (!(T > 0.0)) return PICK_SILENT;
    int S[M], n = 0;
    double w_S[M], res_S[M], before = 1.0;
    for (int k = 0; k < M; k++) { S[k] = -1; w_S[k] = res_S[k] = 0.0; }
    while (n < max_terms) {
        int best = -1;
        double best_res = 0.0, best_w[M];
        for (int c = 0; c < n_candidates; c++) {
            bool in = false;
            for (int k = 0; k < n; k++) in = in || S[k] == candidate[c];
            if (in) continue;
            S[n] = candidate[c];
            double b[M], G[M][M], w[M], res = 0.0;
            for (int j = 0; j <= n; j++) {
                b[j] = g(target, S[j]);
                for (int k = 0; k <= j; k++) G[j][k] = g(S[j], S[k]);
            }
            if (!gdg_fit_solve(n + 1, T, b, G, ridge, w, &res)) continue;        /* skipped, not refused */
            if (best < 0 || res < best_res) {
                best = candidate[c];
                best_res = res;
                for (int k = 0; k <= n; k++) best_w[k] = w[k];
            }
        }
        S[n] = -1;
        if (best < 0 || before - best_res < min_gain) break;
        S[n] = best;
        res_S[n] = before = best_res;
        for (int k = 0; k <= n; k++) w_S[k] = best_w[k];
        n++;
    }
    for (int k = 0; k < M; k++) { picked[k] = S[k]; weight[k] = w_S[k]; residual[k] = res_S[k]; }
    *n_picked = n;
    return PICK_OK;
}

/* ---- the tap fit (include/gdg.h, TAPFIT): a list of fits with T taps per term, the table a launch reads, and the taps from its records
 * (gdg_blend_taps_from_tapfit; tests/native/tapfit_plan_check.cpp) ---------------------------------------------------------------------------- */
#ifndef GDG_TAPFIT_MAX_TERMS
#define GDG_TAPFIT_MAX_TERMS 4
#define GDG_TAPFIT_MAX_UNKNOWNS 128
#define GDG_TAPFIT_MAX_FITS 16
#endif
#define GDG_TAPFIT_TILE 32                                                   /* the kernel's tile of a fit's lower triangle (tapfit_kernels.h) */
/* a fit as the kernel reads it: target | terms | taps | port[4] | where its part of a block's record begins, in doubles | its first tile */
enum { TAPFIT_E_TARGET = 0, TAPFIT_E_TERMS = 1, TAPFIT_E_TAPS = 2, TAPFIT_E_PORT = 3, TAPFIT_E_OFFSET = 3 + GDG_TAPFIT_MAX_TERMS, TAPFIT_E_TILE0, GDG_TAPFIT_TABLE_INTS };

enum {
    TAPFIT_OK = 0,
    TAPFIT_COUNT = 1,                          /* n_fits outside 0 .. GDG_TAPFIT_MAX_FITS */
    TAPFIT_NULL = 2,                           /* a list is missing */
    TAPFIT_FIRST = 3,                          /* first[0] != 0, or first[f + 1] < first[f]: *fit = f */
    TAPFIT_TERMS = 4,                          /* fit f has no term or more than GDG_TAPFIT_MAX_TERMS */
    TAPFIT_TAPS = 5,                           /* fit f has taps outside 1 .. GDG_BLEND_MAX_TAPS */
    TAPFIT_UNKNOWNS = 6,                       /* fit f has more than GDG_TAPFIT_MAX_UNKNOWNS terms x taps */
    TAPFIT_PORT = 7,                           /* term `term` of fit f names a port outside [0, n_ports) */
    TAPFIT_TARGET = 8                          /* fit f's target lies outside [0, n_ports) */
};

/* The list in its CSR form, as the fits': fit f has the terms port[first[f] .. first[f + 1]), the target target[f] and taps[f] taps per term.
 * n_ports < 0: the port count is not known yet and only negative ports are refused.  *fit, *term: the first offender, -1 where none is named. */
static inline int gdg_tapfit_check(int n_fits, const int *first, const int *port, const int *target, const int *taps, int n_ports, int *fit, int *term) {
    *fit = *term = -1;
    if (n_fits < 0 || n_fits > GDG_TAPFIT_MAX_FITS) return TAPFIT_COUNT;
    if (n_fits == 0) return TAPFIT_OK;
    if (!first || !port || !target || !taps) return TAPFIT_NULL;
    if (first[0] != 0) { *fit = 0; return TAPFIT_FIRST; }
    for (int f = 0; f < n_fits; f++) {                                       /* the offsets first: nothing is read through a bad one */
        *fit = f;
        if (first[f + 1] < first[f]) return TAPFIT_FIRST;
        if (first[f + 1] == first[f] || first[f + 1] - first[f] > GDG_TAPFIT_MAX_TERMS) return TAPFIT_TERMS;
        if (taps[f] < 1 || taps[f] > GDG_BLEND_MAX_TAPS) return TAPFIT_TAPS;
        if ((first[f + 1] - first[f]) * taps[f] > GDG_TAPFIT_MAX_UNKNOWNS) return TAPFIT_UNKNOWNS;
    }
    for (int f = 0; f < n_fits; f++) {
        *fit = f;
        if (target[f] < 0 || (n_ports >= 0 && target[f] >= n_ports)) return TAPFIT_TARGET;
        for (int k = first[f]; k < first[f + 1]; k++)
            if (port[k] < 0 || (n_ports >= 0 && port[k] >= n_ports)) { *term = k - first[f]; return TAPFIT_PORT; }
    }
    *fit = -1;
    return TAPFIT_OK;
}

/* V (V + 1) / 2 of one fit, and D of a checked list: the doubles of a block's record */
static inline size_t gdg_tapfit_fit_doubles(int terms, int taps) { const size_t V = (size_t)terms * (size_t)taps + 1; return V * (V + 1) / 2; }
static inline size_t gdg_tapfit_list_doubles(int n_fits, const int *first, const int *taps) {
    size_t D = 0;
    for (int f = 0; f < n_fits; f++) D += gdg_tapfit_fit_doubles(first[f + 1] - first[f], taps[f]);
    return D;
}

/* the list in force, as the table a launch reads */
struct TapFitSet {
    std::vector<int> table;
    int count() const { return (int)(table.size() / GDG_TAPFIT_TABLE_INTS); }
    const int *entry(int f) const { return &table[(size_t)f * GDG_TAPFIT_TABLE_INTS]; }
    int target(int f) const { return entry(f)[TAPFIT_E_TARGET]; }
    int terms(int f) const { return entry(f)[TAPFIT_E_TERMS]; }
    int taps(int f) const { return entry(f)[TAPFIT_E_TAPS]; }
    int port(int f, int k) const { return entry(f)[TAPFIT_E_PORT + k]; }
    size_t doubles() const {                   /* D */
        size_t D = 0;
        for (int f = 0; f < count(); f++) D += gdg_tapfit_fit_doubles(terms(f), taps(f));
        return D;
    }
    /* the first fit that names a port outside [0, n_ports): -1 = none; *term: the term, -1 = the target */
    int first_outside(int n_ports, int *term) const {
        for (int f = 0; f < count(); f++) {
            *term = -1;
            if (target(f) >= n_ports) return f;
            for (int k = 0; k < terms(f); k++) if (port(f, k) >= n_ports) { *term = k; return f; }
        }
        return -1;
    }
};

/* a checked list as a table */
static inline std::vector<int> gdg_tapfit_table(int n_fits, const int *first, const int *port, const int *target, const int *taps) {
    std::vector<int> t((size_t)n_fits * GDG_TAPFIT_TABLE_INTS, 0);
    size_t D = 0;
    int tiles = 0;
    for (int f = 0; f < n_fits; f++) {
        int *e = &t[(size_t)f * GDG_TAPFIT_TABLE_INTS];
        const int K = first[f + 1] - first[f], R = (K * taps[f] + 1 + GDG_TAPFIT_TILE - 1) / GDG_TAPFIT_TILE;
        e[TAPFIT_E_TARGET] = target[f];
        e[TAPFIT_E_TERMS] = K;
        e[TAPFIT_E_TAPS] = taps[f];
        for (int k = 0; k < K; k++) e[TAPFIT_E_PORT + k] = port[first[f] + k];
        e[TAPFIT_E_OFFSET] = (int)D;
        e[TAPFIT_E_TILE0] = tiles;
        D += gdg_tapfit_fit_doubles(K, taps[f]);
        tiles += R * (R + 1) / 2;
    }
    return t;
}

enum {
    TAPS_PLAN_OK = 0,
    TAPS_PLAN_ARGS = 1,                        /* a list is missing, a count or a fit's shape is out of range, no block, ridge is negative or not finite */
    TAPS_PLAN_NONFINITE = 2,                   /* the summed record of *fit has a NaN or inf in virtual row *row */
    TAPS_PLAN_PIVOT = 3                        /* the factorisation of *fit met a pivot at or below the bound in virtual row *row */
};

/* records[blocks][D].  Per fit: the blocks' records added in block order with plain adds; A = G[0 .. U)[0 .. U), b = G[U][0 .. U), Tt = G[U][U];
 * gdg_solve_n on them in virtual-row order.  Every fit is solved before tap (U_f doubles per fit, concatenated) and residual[n_fits] are
 * written; *fit, *row: the offender (term = *row / taps, lag = *row % taps). */
static inline int gdg_blend_plan_taps(const double *records, int n_fits, const int *first, const int *taps, size_t blocks, double ridge, double *tap, double *residual,
                                      int *fit, int *row) {
    *fit = *row = -1;
    if (n_fits < 0 || n_fits > GDG_TAPFIT_MAX_FITS || !(ridge >= 0.0) || !isfinite(ridge)) return TAPS_PLAN_ARGS;
    if (n_fits == 0) return TAPS_PLAN_OK;
    if (!records || !first || !taps || !tap || !residual || blocks == 0 || first[0] != 0) return TAPS_PLAN_ARGS;
    size_t total = 0;
    for (int f = 0; f < n_fits; f++) {
        *fit = f;
        const int K = first[f + 1] - first[f];
        if (K < 1 || K > GDG_TAPFIT_MAX_TERMS || taps[f] < 1 || taps[f] > GDG_BLEND_MAX_TAPS || K * taps[f] > GDG_TAPFIT_MAX_UNKNOWNS) return TAPS_PLAN_ARGS;
        total += (size_t)(K * taps[f]);
    }
    const size_t D = gdg_tapfit_list_doubles(n_fits, first, taps);
    std::vector<double> h_all(total, 0.0), res_all((size_t)n_fits, 0.0), sum, G, Lo, y, b;
    size_t off = 0, at = 0;
    for (int f = 0; f < n_fits; f++) {
        *fit = f;
        const int U = (first[f + 1] - first[f]) * taps[f];
        const size_t E = gdg_tapfit_fit_doubles(first[f + 1] - first[f], taps[f]), ld = (size_t)U;
        sum.assign(E, 0.0);
        for (size_t q = 0; q < blocks; q++) for (size_t e = 0; e < E; e++) sum[e] += records[q * D + off + e];
        for (int i = 0; i <= U; i++)
            for (int j = 0; j <= i; j++) if (!isfinite(sum[gdg_gram_index((size_t)i, (size_t)j)])) { *row = i; return TAPS_PLAN_NONFINITE; }
        G.assign(ld * ld, 0.0);
        Lo.assign(ld * ld, 0.0);
        y.assign(ld, 0.0);
        b.assign(ld, 0.0);
        for (int i = 0; i < U; i++) {
            b[(size_t)i] = sum[gdg_gram_index((size_t)U, (size_t)i)];
            for (int j = 0; j <= i; j++) G[(size_t)i * ld + (size_t)j] = sum[gdg_gram_index((size_t)i, (size_t)j)];
        }
        if (!gdg_solve_n(U, sum[gdg_gram_index((size_t)U, (size_t)U)], b.data(), G.data(), ld, ridge, &h_all[at], &res_all[(size_t)f], row, Lo.data(), y.data())) return TAPS_PLAN_PIVOT;
        off += E;
        at += (size_t)U;
    }
    *fit = *row = -1;
    memcpy(tap, h_all.data(), h_all.size() * sizeof(double));
    memcpy(residual, res_all.data(), res_all.size() * sizeof(double));
    return TAPS_PLAN_OK;
}

/* ---- the transfer records (include/gdg.h, TRANSFER): a list of (port, target) pairs and one group width, the table a launch reads, and the
 * match taps from its records (gdg_match_taps_from_transfer; tests/native/transfer_plan_check.cpp) ------------------------------------------- */
#ifndef GDG_TRANSFER_MAX_PAIRS
#define GDG_TRANSFER_BLOCK 8192
#define GDG_TRANSFER_MAX_PAIRS 16
#define GDG_TRANSFER_MAX_GROUP 64
#endif
/* include/gdg.h states the three for the callers, this file for the code that is compiled without it (fir.hip): they may not drift apart */
static_assert(GDG_TRANSFER_BLOCK == 8192 && GDG_TRANSFER_MAX_PAIRS == 16 && GDG_TRANSFER_MAX_GROUP == 64, "the limits of include/gdg.h, TRANSFER");

enum {
    TRANSFER_OK = 0,
    TRANSFER_COUNT = 1,                        /* n_pairs outside 0 .. GDG_TRANSFER_MAX_PAIRS */
    TRANSFER_NULL = 2,                         /* a list is missing */
    TRANSFER_GROUP = 3,                        /* the group width is not one of 1, 2, 4 .. GDG_TRANSFER_MAX_GROUP */
    TRANSFER_PORT = 4,                         /* pair *pair names a port outside [0, n_ports) */
    TRANSFER_TARGET = 5                        /* pair *pair names a target outside [0, n_ports) */
};

static inline bool gdg_transfer_group_ok(int group) { return group >= 1 && group <= GDG_TRANSFER_MAX_GROUP && !(group & (group - 1)); }

/* the whole list; n_ports < 0: the port count is not known yet.  n_pairs == 0 is a list (off), whatever the group */
static inline int gdg_transfer_check(int n_pairs, const int *port, const int *target, int group, int n_ports, int *pair) {
    *pair = -1;
    if (n_pairs < 0 || n_pairs > GDG_TRANSFER_MAX_PAIRS) return TRANSFER_COUNT;
    if (n_pairs == 0) return TRANSFER_OK;
    if (!port || !target) return TRANSFER_NULL;
    if (!gdg_transfer_group_ok(group)) return TRANSFER_GROUP;
    for (int i = 0; i < n_pairs; i++) {
        *pair = i;
        if (port[i] < 0 || (n_ports >= 0 && port[i] >= n_ports)) return TRANSFER_PORT;
        if (target[i] < 0 || (n_ports >= 0 && target[i] >= n_ports)) return TRANSFER_TARGET;
    }
    *pair = -1;
    return TRANSFER_OK;
}

/* G = 4096 / D + 1 groups of four doubles per pair; 0 for no pair or a width that is none */
static inline size_t gdg_transfer_groups(int group) { return gdg_transfer_group_ok(group) ? (size_t)(GDG_TRANSFER_BLOCK / 2 / group + 1) : 0; }
static inline size_t gdg_transfer_list_doubles(int n_pairs, int group) {
    return n_pairs < 1 || n_pairs > GDG_TRANSFER_MAX_PAIRS ? 0 : (size_t)n_pairs * gdg_transfer_groups(group) * 4;
}

/* the table of a checked list, as a launch reads it: port, target per pair, the group width behind them; no pair: no int */
static inline std::vector<int> gdg_transfer_table(int n_pairs, const int *port, const int *target, int group) {
    std::vector<int> t;
    for (int i = 0; i < n_pairs; i++) { t.push_back(port[i]); t.push_back(target[i]); }
    if (n_pairs > 0) t.push_back(group);
    return t;
}

/* the list in force (ctx.h): its table, empty = off */
struct TransferSet {
    std::vector<int> table;
    int count() const { return table.empty() ? 0 : (int)(table.size() / 2); }
    int group() const { return table.empty() ? 0 : table.back(); }
    int port(int i) const { return table[(size_t)2 * i]; }
    int target(int i) const { return table[(size_t)2 * i + 1]; }
    size_t doubles() const { return gdg_transfer_list_doubles(count(), group()); }
    /* the first pair that names a port at or beyond n_ports; *side: 0 = its port, 1 = its target; -1: none */
    int first_outside(int n_ports, int *side) const {
        for (int i = 0; i < count(); i++) {
            if (port(i) >= n_ports) { *side = 0; return i; }
            if (target(i) >= n_ports) { *side = 1; return i; }
        }
        return -1;
    }
};

/* The inverse real transform of the planner: h[n] = (1 / M) sum_k F[k] exp(+2 pi i k n / M), M = 2 Gm a power of two (128 .. 8192), F the
 * Hermitian extension of H[0 .. Gm] (F[M - k] = conj H[k]; the imaginary parts of H[0] and H[Gm] are not looked at).  The algorithm is
 * the textbook iterative radix-2 decimation-in-time complex transform of length M -- bit-reversed input, log2 M butterfly passes, every
 * twiddle taken from one table of cos and sin evaluated per entry (no recurrence) -- on F; the real parts are the result. */
static inline void gdg_transfer_irfft(const double *Hre, const double *Him, int Gm, double *h) {
    const int M = 2 * Gm;
    const double pi = 3.14159265358979323846;
    std::vector<double> re((size_t)M), im((size_t)M), wr((size_t)Gm), wi((size_t)Gm);
    for (int k = 0; k < Gm; k++) { wr[(size_t)k] = cos(2.0 * pi * (double)k / (double)M); wi[(size_t)k] = sin(2.0 * pi * (double)k / (double)M); }
    int bits = 0;
    while ((1 << bits) < M) bits++;
    for (int k = 0; k < M; k++) {
        int r = 0;
        for (int b = 0; b < bits; b++) if (k & (1 << b)) r |= 1 << (bits - 1 - b);
        double a, c;
        if (k == 0 || k == Gm) { a = Hre[k]; c = 0.0; }
        else if (k < Gm) { a = Hre[k]; c = Him[k]; }
        else { a = Hre[M - k]; c = -Him[M - k]; }
        re[(size_t)r] = a;
        im[(size_t)r] = c;
    }
    for (int len = 2; len <= M; len <<= 1) {
        const int half = len / 2, step = M / len;
        for (int s = 0; s < M; s += len)
            for (int j = 0; j < half; j++) {
                const double cr = wr[(size_t)(j * step)], ci = wi[(size_t)(j * step)];
                const size_t u = (size_t)(s + j), v = u + (size_t)half;
                const double tr = re[v] * cr - im[v] * ci, ti = re[v] * ci + im[v] * cr;
                re[v] = re[u] - tr; im[v] = im[u] - ti;
                re[u] = re[u] + tr; im[u] = im[u] + ti;
            }
    }
    for (int n = 0; n < M; n++) h[n] = re[(size_t)n] / (double)M;
}

enum {
    MATCH_PLAN_OK = 0,
    MATCH_PLAN_ARGS = 1,                       /* a list is missing, a count, the group, n_taps or center is out of range, no block, ridge is negative or not finite */
    MATCH_PLAN_NONFINITE = 2,                  /* the summed record of *pair has a NaN or inf entry */
    MATCH_PLAN_SILENT = 3                      /* the summed record of *pair has no energy in the port: every Sxx[g] is 0 */
};

/* records[blocks][n_pairs][G][4] (Sxx, Syy, Re Sxy, Im Sxy).  Per pair: the blocks' records added in block order with plain adds; N' = 2 Gm;
 * H[g] = Sxy[g] / (Sxx[g] + ridge * mean_g Sxx), 0 where that denominator is 0; h = gdg_transfer_irfft(H); tap[m] = t[m] h[(m - center) mod
 * N'] with the raised-cosine taper t (1 at the centre, E = center + 1 in front, n_taps - center behind: never 0 inside); coherence =
 * sum_g (|Sxy[g]|^2 / Sxx[g]) / sum_g Syy[g] over the groups with Sxx[g] > 0, 0 when sum Syy is 0.  Every pair is planned before
 * tap[n_pairs][n_taps] and coherence[n_pairs] are written; *pair: the offender. */
static inline int gdg_match_plan_taps(const double *records, int n_pairs, int group, size_t blocks, double ridge, int n_taps, int center, double *tap, double *coherence,
                                      int *pair) {
    *pair = -1;
    if (n_pairs < 0 || n_pairs > GDG_TRANSFER_MAX_PAIRS || !(ridge >= 0.0) || !isfinite(ridge) || !gdg_transfer_group_ok(group)) return MATCH_PLAN_ARGS;
    const int Gm = GDG_TRANSFER_BLOCK / 2 / group, G = Gm + 1, M = 2 * Gm;
    if (n_taps < 1 || n_taps > M / 2 || center < 0 || center >= n_taps) return MATCH_PLAN_ARGS;
    if (n_pairs == 0) return MATCH_PLAN_OK;
    if (!records || !tap || !coherence || blocks == 0) return MATCH_PLAN_ARGS;
    const double pi = 3.14159265358979323846;
    const size_t per = (size_t)n_pairs * (size_t)G * 4;
    std::vector<double> tap_all((size_t)n_pairs * (size_t)n_taps, 0.0), coh_all((size_t)n_pairs, 0.0), sum((size_t)G * 4), Hre((size_t)G), Him((size_t)G), h((size_t)M);
    for (int p = 0; p < n_pairs; p++) {
        *pair = p;
        sum.assign((size_t)G * 4, 0.0);
        for (size_t q = 0; q < blocks; q++) for (size_t e = 0; e < (size_t)G * 4; e++) sum[e] += records[q * per + (size_t)p * (size_t)G * 4 + e];
        double total = 0.0, syy = 0.0, explained = 0.0;
        for (int g = 0; g < G; g++) {
            for (int c = 0; c < 4; c++) if (!isfinite(sum[(size_t)g * 4 + c])) return MATCH_PLAN_NONFINITE;
            total += sum[(size_t)g * 4];
        }
        if (!(total > 0.0)) return MATCH_PLAN_SILENT;
        const double load = ridge * (total / (double)G);
        for (int g = 0; g < G; g++) {
            const double sxx = sum[(size_t)g * 4], re = sum[(size_t)g * 4 + 2], im = sum[(size_t)g * 4 + 3], den = sxx + load;
            Hre[(size_t)g] = den != 0.0 ? re / den : 0.0;
            Him[(size_t)g] = den != 0.0 ? im / den : 0.0;
            syy += sum[(size_t)g * 4 + 1];
            if (sxx > 0.0) explained += (re * re + im * im) / sxx;
        }
        gdg_transfer_irfft(Hre.data(), Him.data(), Gm, h.data());
        for (int m = 0; m < n_taps; m++) {
            const int d = m - center;
            const double E = d < 0 ? (double)(center + 1) : (double)(n_taps - center);
            const double t = 0.5 + 0.5 * cos(pi * (double)d / E);
            tap_all[(size_t)p * (size_t)n_taps + (size_t)m] = t * h[(size_t)((d + M) % M)];
        }
        coh_all[(size_t)p] = syy > 0.0 ? explained / syy : 0.0;
    }
    *pair = -1;
    memcpy(tap, tap_all.data(), tap_all.size() * sizeof(double));
    memcpy(coherence, coh_all.data(), coh_all.size() * sizeof(double));
    return MATCH_PLAN_OK;
}

#endif
