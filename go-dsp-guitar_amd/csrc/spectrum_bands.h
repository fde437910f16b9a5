/*
 * spectrum_bands.h -- the host side of the band spectrum (include/gdg.h, gdg_block_spectrum_rows): the edge list's validation and the
 * first bin of every band.  Plain C++, no device and no context: tests/native/spectrum_check.cpp drives it under AddressSanitizer and UBSan.
 */
#pragma once
#include <math.h>
#include <stdint.h>

#define GDG_SPECTRUM_BLOCK 8192               /* L: the samples of a block = the length of the transform */
#define GDG_SPECTRUM_BINS (GDG_SPECTRUM_BLOCK / 2 + 1)      /* k = 0 .. L/2 */
#define GDG_SPECTRUM_MAX_EDGES 33             /* at most 32 bands */

/* what the kernel is given by value: band b holds the bins k_lo[b] <= k < k_lo[b + 1] */
struct gdg_spectrum_bands {
    int n_bands;
    int k_lo[GDG_SPECTRUM_MAX_EDGES];
};

enum { SPECTRUM_OK = 0, SPECTRUM_COUNT = 1, SPECTRUM_NULL = 2, SPECTRUM_VALUE = 3, SPECTRUM_ORDER = 4 };

/* 2 <= n_edges <= 33 edges: finite, >= 0, strictly ascending; *bad: the first offending edge, -1 when the list as a whole is refused */
static inline int spectrum_edges_check(const double *edges_hz, int n_edges, int *bad) {
    *bad = -1;
    if (n_edges < 2 || n_edges > GDG_SPECTRUM_MAX_EDGES) return SPECTRUM_COUNT;
    if (!edges_hz) return SPECTRUM_NULL;
    for (int i = 0; i < n_edges; i++) {
        const double e = edges_hz[i];
        if (!(e >= 0.0) || !(e <= 1.7976931348623157e308)) { *bad = i; return SPECTRUM_VALUE; }      /* NaN fails the first test, +inf the second */
        if (i > 0 && !(e > edges_hz[i - 1])) { *bad = i; return SPECTRUM_ORDER; }
    }
    return SPECTRUM_OK;
}

/* k_lo = clamp((long long)ceil(edge * 8192.0 / R), 0, 4097), in float64 as written.  The quotient is compared before it is converted: an
 * edge far above Nyquist (or an overflowing product) never reaches a conversion it does not fit */
static inline int spectrum_k_lo(double edge_hz, uint32_t sample_rate) {
    const double k = ceil(edge_hz * 8192.0 / (double)sample_rate);
    if (!(k > 0.0)) return 0;
    if (k >= (double)GDG_SPECTRUM_BINS) return GDG_SPECTRUM_BINS;
    return (int)(long long)k;
}

/* a checked edge list at a positive rate -> the kernel's argument */
static inline gdg_spectrum_bands spectrum_bands(const double *edges_hz, int n_edges, uint32_t sample_rate) {
    gdg_spectrum_bands b;
    b.n_bands = n_edges - 1;
    for (int i = 0; i < GDG_SPECTRUM_MAX_EDGES; i++) b.k_lo[i] = GDG_SPECTRUM_BINS;
    for (int i = 0; i < n_edges; i++) b.k_lo[i] = spectrum_k_lo(edges_hz[i], sample_rate);
    return b;
}

/* the periodic Hann window, w[n] = 0.5 - 0.5 cos(2 pi n / L) */
static inline void spectrum_window(double *w) {
    for (int n = 0; n < GDG_SPECTRUM_BLOCK; n++) w[n] = 0.5 - 0.5 * cos(2.0 * 3.14159265358979323846 * (double)n / (double)GDG_SPECTRUM_BLOCK);
}
