/*
 * blend.h -- the blend outputs (gdg_batch_set_blends, gdg_blend_rows; include/gdg.h states the arithmetic): a blend is a weighted sum of
 * chain output rows, s = w_0 x[c_0], then s = s + w_k x[c_k] in term order, every product and every add rounded on its own.  Here: the two
 * rounded operations as __host__ __device__ inlines -- the kernel of blend_kernels.h uses them, and so can a stand-alone host program
 * (tests/native/blend_check.cpp) -- the validation of a blend list in its CSR form, the rule by which a list replaces the one in force, and
 * the sum on the host.  No HIP header is needed to compile this file.
 */
#ifndef GDG_BLEND_H
#define GDG_BLEND_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

/* the limits of include/gdg.h */
#ifndef GDG_BLEND_MAX_TERMS
#define GDG_BLEND_MAX_TERMS 32
#define GDG_BLEND_MAX_BLENDS 1024
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
    BLEND_GAIN = 8                             /* blend b's output gain is not finite */
};

/* The whole list: n_blends blends, blend b's terms at [first[b], first[b + 1]) of channel[] and weight[]; gain: one per blend, or null (all
 * 1.0).  *blend, *term: the first offender (the term counted within its blend), -1 where the status names none. */
static inline int gdg_blend_check(int n_blends, const int *first, const int *channel, const double *weight, const double *gain, int n_channels,
                                  int *blend, int *term) {
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
        }
        *term = -1;
        if (gain && !isfinite(gain[b])) return BLEND_GAIN;
    }
    *blend = -1;
    return BLEND_OK;
}

/* the list in force */
struct BlendSet {
    std::vector<int> first, channel;           /* first: count() + 1 offsets, empty = off */
    std::vector<double> weight, gain;          /* gain: one per blend, 1.0 where none was given */
    int count() const { return first.empty() ? 0 : (int)first.size() - 1; }
    int terms() const { return (int)channel.size(); }
    bool unit_gains() const { for (double g : gain) if (g != 1.0) return false; return true; }
    /* the table as a batch call uploads it, made when the list is taken: first | channel | pad to 8 bytes | weight | gain */
    std::vector<unsigned char> packed;
    size_t packed_ints() const { return ((first.size() + channel.size()) * sizeof(int) + 7) & ~(size_t)7; }
    void pack() {
        packed.assign(first.empty() ? 0 : packed_ints() + (weight.size() + gain.size()) * sizeof(double), 0);
        if (packed.empty()) return;
        memcpy(packed.data(), first.data(), first.size() * sizeof(int));
        memcpy(packed.data() + first.size() * sizeof(int), channel.data(), channel.size() * sizeof(int));
        memcpy(packed.data() + packed_ints(), weight.data(), weight.size() * sizeof(double));
        memcpy(packed.data() + packed_ints() + weight.size() * sizeof(double), gain.data(), gain.size() * sizeof(double));
    }
};

/* whole or not at all: a refused list leaves the one in force as it is */
static inline int gdg_blend_replace(BlendSet &set, int n_blends, const int *first, const int *channel, const double *weight, const double *gain,
                                    int n_channels, int *blend, int *term) {
    const int rc = gdg_blend_check(n_blends, first, channel, weight, gain, n_channels, blend, term);
    if (rc != BLEND_OK) return rc;
    BlendSet next;
    if (n_blends > 0) {
        const int terms = first[n_blends];
        next.first.assign(first, first + n_blends + 1);
        next.channel.assign(channel, channel + terms);
        next.weight.assign(weight, weight + terms);
        if (gain) next.gain.assign(gain, gain + n_blends);
        else next.gain.assign((size_t)n_blends, 1.0);
    }
    next.pack();
    set = next;
    return BLEND_OK;
}

/* the definition on the host: sample i of the blend with terms [k0, k1) over rows[channel][i] */
static inline double gdg_blend_sample(const double *const *rows, size_t i, const int *channel, const double *weight, int k0, int k1) {
    double s = gdg_blend_mul(weight[k0], rows[channel[k0]][i]);
    for (int k = k0 + 1; k < k1; k++) s = gdg_blend_add(s, gdg_blend_mul(weight[k], rows[channel[k]][i]));
    return s;
}

/* a checked list over `samples` samples of every row: out[b][i] */
static inline void gdg_blend_sum_host(const double *const *rows, size_t samples, int n_blends, const int *first, const int *channel, const double *weight,
                                      double *const *out) {
    for (int b = 0; b < n_blends; b++)
        for (size_t i = 0; i < samples; i++) out[b][i] = gdg_blend_sample(rows, i, channel, weight, first[b], first[b + 1]);
}

#endif
