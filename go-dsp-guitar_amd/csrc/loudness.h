/*
 * loudness.h -- the host arithmetic of the loudness records (include/gdg.h, LOUDNESS): the K-weighting's coefficients at any
 * rate, what a launch of block_loudness_kernel (loudness_kernels.h) takes as its uniform argument, the count of hops a span of samples
 * completes, and the two planners that turn hop records into LUFS figures and gains.  Pure float64 on the host; no HIP header is needed to
 * compile this file (tests/native/loudness_check.cpp does so).
 */
#ifndef GDG_LOUDNESS_H
#define GDG_LOUDNESS_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "trim.h"

#define LOUDNESS_TILE 8192                     /* samples of a tile, counted from the job's start: a block of the batch loop */
#define LOUDNESS_CHUNK 32                      /* samples one thread runs sequentially */
#define LOUDNESS_CHUNKS (LOUDNESS_TILE / LOUDNESS_CHUNK)
#define LOUDNESS_CELL 64                       /* squares summed sequentially, counted from the hop's start */
#define LOUDNESS_LEVELS 8                      /* the scan over a tile's 256 chunks: distances 1, 2 .. 128 */
#define LOUDNESS_STATE 7                       /* GDG_LOUDNESS_STATE_DOUBLES: s0, s1, q0, q1, the open cell's sum, the open hop's sum, the position */

/* the two stages of BS.1770's pre-filter as the analogue prototypes they were made from, so that every rate gets its own coefficients */
#define LOUDNESS_SHELF_F0 1681.974450955533
#define LOUDNESS_SHELF_Q 0.7071752369554196
#define LOUDNESS_SHELF_DB 3.999843853973347
#define LOUDNESS_SHELF_VB_EXP 0.4996667741545416
#define LOUDNESS_HP_F0 38.13547087602444
#define LOUDNESS_HP_Q 0.5003270373238773
#define LOUDNESS_PI 3.14159265358979323846

/* What a launch reads, uniform: the shelf's b0 b1 b2 a1 a2, the high-pass' alpha and beta (below), and P[k] = A^(32 * 2^k), row-major, A the
 * one-sample map of the four states at input 0 */
struct gdg_loudness_params {
    double shelf[5];
    double alpha, beta;
    double P[LOUDNESS_LEVELS][16];
};

/* a rate the records are defined at: a hop is rate / 10 samples, whole, and at least 800 of them */
static inline bool gdg_loudness_rate_ok(uint32_t rate) { return rate >= 8000 && rate % 10 == 0; }
static inline uint64_t gdg_loudness_hop(uint32_t rate) { return rate / 10; }

/* hops that complete in the samples [first, first + count) of a job */
static inline uint64_t gdg_loudness_hops_in(uint32_t rate, uint64_t first, uint64_t count) {
    const uint64_t H = gdg_loudness_hop(rate);
    return (first + count) / H - first / H;
}

/* out[10]: shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2 (a0 = 1), by include/gdg.h's formulas */
static inline void gdg_loudness_coefficients_at(double rate, double out[10]) {
    {
        const double K = tan(LOUDNESS_PI * LOUDNESS_SHELF_F0 / rate), Q = LOUDNESS_SHELF_Q;
        const double Vh = pow(10.0, LOUDNESS_SHELF_DB / 20.0), Vb = pow(Vh, LOUDNESS_SHELF_VB_EXP);
        const double a0 = 1.0 + K / Q + K * K;
        out[0] = (Vh + Vb * K / Q + K * K) / a0;
        out[1] = 2.0 * (K * K - Vh) / a0;
        out[2] = (Vh - Vb * K / Q + K * K) / a0;
        out[3] = 2.0 * (K * K - 1.0) / a0;
        out[4] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double K = tan(LOUDNESS_PI * LOUDNESS_HP_F0 / rate), Q = LOUDNESS_HP_Q;
        const double a0 = 1.0 + K / Q + K * K;
        out[5] = 1.0;
        out[6] = -2.0;
        out[7] = 1.0;
        out[8] = 2.0 * (K * K - 1.0) / a0;
        out[9] = (1.0 - K / Q + K * K) / a0;
    }
}

/* The high-pass' poles lie within 0.3 % of z = 1, where a1 = -2 + beta and a2 = 1 + alpha - beta lose what alpha and beta say: the stage
 * runs on alpha = 1 + a1 + a2 = 4 K^2 / a0 and beta = 2 + a1 = (2 K / Q + 4 K^2) / a0, made from K and Q without the subtraction */
static inline void gdg_loudness_hp_delta(double rate, double *alpha, double *beta) {
    const double K = tan(LOUDNESS_PI * LOUDNESS_HP_F0 / rate), Q = LOUDNESS_HP_Q;
    const double a0 = 1.0 + K / Q + K * K;
    *alpha = 4.0 * K * K / a0;
    *beta = (2.0 * K / Q + 4.0 * K * K) / a0;
}

static inline void gdg_loudness_mat_mul(const double *a, const double *b, double *out) {
    double r[16];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double acc = 0.0;
            for (int k = 0; k < 4; k++) acc += a[4 * i + k] * b[4 * k + j];
            r[4 * i + j] = acc;
        }
    for (int i = 0; i < 16; i++) out[i] = r[i];
}

/* the launch argument at `rate`: the states are (s0, s1) of the shelf in transposed direct form II and (q0, q1) of the high-pass (include/gdg.h
 * states the recurrence); at input 0 they map by A, and a chunk of 32 samples by A^32 */
static inline gdg_loudness_params gdg_loudness_params_at(uint32_t rate) {
    gdg_loudness_params p;
    double c[10];
    gdg_loudness_coefficients_at((double)rate, c);
    for (int i = 0; i < 5; i++) p.shelf[i] = c[i];
    gdg_loudness_hp_delta((double)rate, &p.alpha, &p.beta);
    const double a1 = c[3], a2 = c[4], al = p.alpha, be = p.beta;
    double A[16] = { -a1, 1.0, 0.0, 0.0,
                     -a2, 0.0, 0.0, 0.0,
                     -be, 0.0, 1.0 - be, 1.0,
                     -al, 0.0, -al, 1.0 };
    for (int k = 0; k < 5; k++) gdg_loudness_mat_mul(A, A, A);                 /* A^32 */
    for (int k = 0; k < LOUDNESS_LEVELS; k++) {
        for (int i = 0; i < 16; i++) p.P[k][i] = A[i];
        gdg_loudness_mat_mul(A, A, A);
    }
    return p;
}

/* ---- the planners (include/gdg.h, LOUDNESS: gdg_loudness_from_hops, gdg_trim_from_loudness) ------------------------------------------- */
enum { GDG_LOUDNESS_PLAN_OK = 0, GDG_LOUDNESS_PLAN_ARGS = 1, GDG_LOUDNESS_PLAN_RATE = 2, GDG_LOUDNESS_PLAN_PORT = 3, GDG_LOUDNESS_PLAN_WEIGHT = 4, GDG_LOUDNESS_PLAN_RECORD = 5,
       GDG_LOUDNESS_PLAN_TARGET = 6, GDG_LOUDNESS_PLAN_CEILING = 7, GDG_LOUDNESS_PLAN_PEAK = 8 };

#define LOUDNESS_OFFSET (-0.691)
#define LOUDNESS_ABSOLUTE_GATE (-70.0)
#define LOUDNESS_RELATIVE_GATE (-10.0)
#define LOUDNESS_BLOCK_HOPS 4                  /* a gating block: 400 ms on the 100 ms hop */
#define LOUDNESS_SHORT_HOPS 30                 /* the short-term window: 3 s */

static inline double gdg_loudness_lufs(double power) { return power > 0.0 ? LOUDNESS_OFFSET + 10.0 * log10(power) : -INFINITY; }

/* records[p * n_hops + h]: port p's sum of squares over hop h.  The programme is the n listed ports with their weights; its power over a hop
 * is sum_i weight[i] * records[port[i]][h] / H.  A block is four consecutive hops (block j = hops j .. j + 3), its power their mean.
 * integrated: mean of the blocks above -70 LUFS and above the mean of those minus 10 LU; momentary_max: the largest block; short_term_max:
 * the largest mean of 30 consecutive hops; -inf where there is none.  *bad: the entry or record that was refused. */
static inline int gdg_loudness_plan(const double *records, int n_ports, size_t n_hops, uint32_t rate, const int *port, const double *weight, int n, double *integrated,
                                    double *momentary_max, double *short_term_max, long long *bad) {
    if (n_ports <= 0 || n <= 0 || !port || (!records && n_hops > 0)) return GDG_LOUDNESS_PLAN_ARGS;
    if (!gdg_loudness_rate_ok(rate)) return GDG_LOUDNESS_PLAN_RATE;
    for (int i = 0; i < n; i++) {
        if (port[i] < 0 || port[i] >= n_ports) { if (bad) *bad = i; return GDG_LOUDNESS_PLAN_PORT; }
        if (weight && (!isfinite(weight[i]) || weight[i] < 0.0)) { if (bad) *bad = i; return GDG_LOUDNESS_PLAN_WEIGHT; }
    }
    const double H = (double)gdg_loudness_hop(rate);
    std::vector<double> z(n_hops, 0.0);
    for (int i = 0; i < n; i++)
        for (size_t h = 0; h < n_hops; h++) {
            const double v = records[(size_t)port[i] * n_hops + h];
            if (!(v >= 0.0) || !isfinite(v)) { if (bad) *bad = (long long)((size_t)port[i] * n_hops + h); return GDG_LOUDNESS_PLAN_RECORD; }
            z[h] += (weight ? weight[i] : 1.0) * v / H;
        }
    double mom = 0.0, sht = 0.0, gated = -INFINITY;
    const size_t n_blocks = n_hops >= LOUDNESS_BLOCK_HOPS ? n_hops - LOUDNESS_BLOCK_HOPS + 1 : 0;
    std::vector<double> block(n_blocks);
    for (size_t j = 0; j < n_blocks; j++) {
        block[j] = (((z[j] + z[j + 1]) + z[j + 2]) + z[j + 3]) / (double)LOUDNESS_BLOCK_HOPS;
        if (block[j] > mom) mom = block[j];
    }
    for (size_t j = 0; j + LOUDNESS_SHORT_HOPS <= n_hops; j++) {
        double acc = 0.0;
        for (int k = 0; k < LOUDNESS_SHORT_HOPS; k++) acc += z[j + k];
        acc /= (double)LOUDNESS_SHORT_HOPS;
        if (acc > sht) sht = acc;
    }
    const double abs_gate = pow(10.0, (LOUDNESS_ABSOLUTE_GATE - LOUDNESS_OFFSET) / 10.0);
    double sum = 0.0;
    size_t count = 0;
    for (size_t j = 0; j < n_blocks; j++) if (block[j] > abs_gate) { sum += block[j]; count++; }
    if (count) {
        const double rel_gate = sum / (double)count * pow(10.0, LOUDNESS_RELATIVE_GATE / 10.0);
        double sum2 = 0.0;
        size_t count2 = 0;
        for (size_t j = 0; j < n_blocks; j++) if (block[j] > abs_gate && block[j] > rel_gate) { sum2 += block[j]; count2++; }
        if (count2) gated = gdg_loudness_lufs(sum2 / (double)count2);
    }
    if (integrated) *integrated = gated;
    if (momentary_max) *momentary_max = gdg_loudness_lufs(mom);
    if (short_term_max) *short_term_max = gdg_loudness_lufs(sht);
    return GDG_LOUDNESS_PLAN_OK;
}

/* One gain per port toward target_lufs: 10^((target - L) / 20) with L the port's own integrated loudness at weight 1, and 1 for a port
 * without one.  With true-peak records ([n_ports][tp_blocks], two doubles a record, true_peak first) the gain is capped by
 * gdg_trim_from_true_peak's rule at the ceiling: min(ceiling / m, gain), m the port's largest true peak; capped[p] says whether it was.
 * Nothing of gain or capped is written unless the whole plan is good. */
static inline int gdg_loudness_trim_plan(const double *records, int n_ports, size_t n_hops, uint32_t rate, double target_lufs, double ceiling_dbtp, const double *true_peak,
                                         size_t tp_blocks, double *gain, int *capped, long long *bad) {
    if (n_ports <= 0 || !gain || (!records && n_hops > 0)) return GDG_LOUDNESS_PLAN_ARGS;
    if (!gdg_loudness_rate_ok(rate)) return GDG_LOUDNESS_PLAN_RATE;
    if (!isfinite(target_lufs)) return GDG_LOUDNESS_PLAN_TARGET;
    if (true_peak && !isfinite(ceiling_dbtp)) return GDG_LOUDNESS_PLAN_CEILING;
    std::vector<double> g((size_t)n_ports, 1.0);
    std::vector<int> cap((size_t)n_ports, 0);
    const double ceiling = pow(10.0, ceiling_dbtp / 20.0);
    for (int p = 0; p < n_ports; p++) {
        double L = -INFINITY;
        const double one = 1.0;
        const int rc = gdg_loudness_plan(records, n_ports, n_hops, rate, &p, &one, 1, &L, nullptr, nullptr, bad);
        if (rc != GDG_LOUDNESS_PLAN_OK) return rc;
        if (isfinite(L)) g[(size_t)p] = pow(10.0, (target_lufs - L) / 20.0);
        if (!true_peak || tp_blocks == 0 || !isfinite(g[(size_t)p]) || !(g[(size_t)p] > 0.0)) continue;
        double capped_gain = g[(size_t)p];
        int bad_port = -1;
        if (gdg_trim_plan(true_peak + (size_t)p * tp_blocks * 2, 2, 1, tp_blocks, ceiling, g[(size_t)p], &capped_gain, &bad_port) != GDG_TRIM_PLAN_OK) {
            if (bad) *bad = p;
            return GDG_LOUDNESS_PLAN_PEAK;
        }
        double m = 0.0;
        for (size_t b = 0; b < tp_blocks; b++) if (true_peak[((size_t)p * tp_blocks + b) * 2] > m) m = true_peak[((size_t)p * tp_blocks + b) * 2];
        if (m > 0.0 && capped_gain < g[(size_t)p]) { g[(size_t)p] = capped_gain; cap[(size_t)p] = 1; }
    }
    for (int p = 0; p < n_ports; p++) { gain[p] = g[(size_t)p]; if (capped) capped[p] = cap[(size_t)p]; }
    return GDG_LOUDNESS_PLAN_OK;
}

#endif
