/*
 * trim.h -- the output trim (gdg_batch_set_trim, include/gdg.h states the arithmetic): one gain per output port in front of the encoders,
 * y = x * g rounded once, and then whatever the encoder does with a sample.  Here: the product as a __host__ __device__ inline -- the trim
 * kernels of io.hip use it, and so can a stand-alone host program (tests/native/trim_check.cpp) -- and the pure host arithmetic behind the
 * configuration: the check of a gain list, whether a setting is "off", and the planner that turns true-peak records into gains
 * (gdg_trim_from_true_peak).  No HIP header is needed to compile this file.
 */
#ifndef GDG_TRIM_H
#define GDG_TRIM_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GDG_TRIM_HD __host__ __device__ __forceinline__
#else
#define GDG_TRIM_HD static inline
#endif

/* the product is rounded before anything else sees it: never contracted with the encoder's scale, on any compiler */
#if defined(__HIP_DEVICE_COMPILE__)
#define GDG_TRIM_MUL(a, b) __dmul_rn((a), (b))
#else
static inline double gdg_trim_mul_(double a, double b) { volatile double r = a * b; return r; }
#define GDG_TRIM_MUL(a, b) gdg_trim_mul_((a), (b))
#endif

/* y = fl(x * g): what the encoder is given in the place of x */
GDG_TRIM_HD double gdg_trim_apply(double x, double g) { return GDG_TRIM_MUL(x, g); }

/* ---- the configuration's arithmetic (host) --------------------------------------------------------------------------------------------- */
/* the job-wide gains sit behind the chain gains in the files' order: master left, master right, metronome (the rows of a batch window) */
#define GDG_TRIM_MASTER_LEFT  0
#define GDG_TRIM_MASTER_RIGHT 1
#define GDG_TRIM_METRONOME    2

/* the first entry of gain[0 .. n) that is not finite, -1 when every one is */
static inline int gdg_trim_first_nonfinite(const double *gain, int n) {
    for (int i = 0; i < n; i++) if (!isfinite(gain[i])) return i;
    return -1;
}

/* every gain exactly 1.0: the setting is "off" */
static inline bool gdg_trim_all_unit(const double *gain, int n) {
    for (int i = 0; i < n; i++) if (gain[i] != 1.0) return false;
    return true;
}

/* what the planner refuses */
enum { GDG_TRIM_PLAN_OK = 0, GDG_TRIM_PLAN_ARGS = 1, GDG_TRIM_PLAN_TARGET = 2, GDG_TRIM_PLAN_MAX_GAIN = 3, GDG_TRIM_PLAN_NAN = 4 };

/* The planner: true_peak[(p * blocks + b) * step] for port p < ports and block b < blocks (a gdg_block_true_peak is two doubles wide: its
 * true_peak fields lie step = 2 apart).  m = the largest of a port's blocks; gain = 1 for a silent port, else min(target / m, max_gain).
 * A NaN true_peak: GDG_TRIM_PLAN_NAN with *bad = the port; nothing of `gain` is written unless the whole plan is good. */
static inline int gdg_trim_plan(const double *true_peak, size_t step, int ports, size_t blocks, double target, double max_gain, double *gain, int *bad) {
    if (ports < 0 || !gain || (!true_peak && ports > 0 && blocks > 0)) return GDG_TRIM_PLAN_ARGS;
    if (!isfinite(target) || !(target > 0.0)) return GDG_TRIM_PLAN_TARGET;
    if (!isfinite(max_gain) || !(max_gain > 0.0)) return GDG_TRIM_PLAN_MAX_GAIN;
    for (int p = 0; p < ports; p++)
        for (size_t b = 0; b < blocks; b++)
            if (isnan(true_peak[((size_t)p * blocks + b) * step])) { if (bad) *bad = p; return GDG_TRIM_PLAN_NAN; }
    for (int p = 0; p < ports; p++) {
        double m = 0.0;
        for (size_t b = 0; b < blocks; b++) { const double v = true_peak[((size_t)p * blocks + b) * step]; if (v > m) m = v; }
        if (m == 0.0) { gain[p] = 1.0; continue; }
        const double g = target / m;
        gain[p] = g < max_gain ? g : max_gain;
    }
    return GDG_TRIM_PLAN_OK;
}

#endif
