/*
 * true_peak_taps.h -- the host side of the true-peak record (include/gdg.h, gdg_block_true_peak_rows): the 3 x 24 interpolation taps of the
 * 4x oversampled reading, built in float64, and the range of sample intervals a block of a given length evaluates.  Plain C++, no device
 * and no context: tests/native/true_peak_check.cpp drives it under AddressSanitizer and UBSan.
 */
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#define GDG_TRUE_PEAK_BLOCK 8192              /* L: the samples of a block */
#define GDG_TRUE_PEAK_OS 4                    /* the oversampling factor: phases 1, 2, 3 lie between two samples */
#define GDG_TRUE_PEAK_H 12                    /* the half-width: a point reads the samples n - H + 1 .. n + H */
#define GDG_TRUE_PEAK_PHASES (GDG_TRUE_PEAK_OS - 1)
#define GDG_TRUE_PEAK_TAPS (2 * GDG_TRUE_PEAK_H)

/* what the kernel is given by value: h[phase - 1][j + H - 1] for j = -H + 1 .. H */
struct gdg_true_peak_table {
    double h[GDG_TRUE_PEAK_PHASES][GDG_TRUE_PEAK_TAPS];
};

/* g[j] = sinc(t) (0.5 + 0.5 cos(pi t / H)), t = phase / 4 - j; h[j] = g[j] / sum_j g[j], the sum added in ascending j: every phase sums to
 * 1, so a constant is reproduced.  t is never 0 (the phase is 1, 2 or 3) and |t| < H */
static inline void true_peak_build(gdg_true_peak_table *table) {
    const double pi = 3.14159265358979323846;
    for (int p = 1; p <= GDG_TRUE_PEAK_PHASES; p++) {
        double g[GDG_TRUE_PEAK_TAPS], sum = 0.0;
        for (int j = -GDG_TRUE_PEAK_H + 1; j <= GDG_TRUE_PEAK_H; j++) {
            const double t = (double)p / (double)GDG_TRUE_PEAK_OS - (double)j;
            g[j + GDG_TRUE_PEAK_H - 1] = sin(pi * t) / (pi * t) * (0.5 + 0.5 * cos(pi * t / (double)GDG_TRUE_PEAK_H));
        }
        for (int k = 0; k < GDG_TRUE_PEAK_TAPS; k++) sum += g[k];
        for (int k = 0; k < GDG_TRUE_PEAK_TAPS; k++) table->h[p - 1][k] = g[k] / sum;
    }
}

/* the table into `taps` ([3][24], row-major); false when there is no room for its 72 entries */
static inline bool true_peak_copy(const gdg_true_peak_table *table, double *taps, int capacity) {
    if (!taps || capacity < GDG_TRUE_PEAK_PHASES * GDG_TRUE_PEAK_TAPS) return false;
    for (int p = 0; p < GDG_TRUE_PEAK_PHASES; p++)
        for (int k = 0; k < GDG_TRUE_PEAK_TAPS; k++) taps[p * GDG_TRUE_PEAK_TAPS + k] = table->h[p][k];
    return true;
}

/* a block of `len` samples evaluates the intervals behind the samples n = *first .. *first + *count - 1: those whose 24 samples
 * n - H + 1 .. n + H all lie inside the block.  len < 24: none */
static inline void true_peak_range(size_t len, size_t *first, size_t *count) {
    *first = GDG_TRUE_PEAK_H - 1;
    *count = len >= (size_t)GDG_TRUE_PEAK_TAPS ? len - (size_t)GDG_TRUE_PEAK_TAPS + 1 : 0;
}
