/*
 * deliver.h -- the delivery of batch outputs at a half or a quarter of the session rate, and at a rational ratio L / M behind that (include/gdg.h,
 * DELIVERY): the factor's and the ratio's rules and the
 * ONE statement of the byte counts of a delivered step.  Every port that leaves the device encoded has samples / R samples (times L / M, counted
 * in job indices, with a ratio), so whatever a
 * step derives from "w blocks times the sample width" -- a row's bytes, where its bytes lie in the file, the pieces of the download, where
 * the record sections begin behind the rows -- is derived here, from the delivered length.  R = 1 gives the figures the block loop always had.
 * Pure host arithmetic: no HIP header is needed to compile this file (tests/native/deliver_bytes_check.cpp holds it against plain formulas).
 */
#ifndef GDG_DELIVER_H
#define GDG_DELIVER_H

#include <stddef.h>

#define GDG_DELIVER_BLOCK 8192                       /* a block of the batch loop, in session samples */
#define GDG_DELIVER_HISTORY 154                      /* session samples a port keeps from step to step: the longer filter's reach, T - 1 of R = 4 */
#define GDG_DELIVER_ATTENUATION 0.9440608762859234   /* ATTENUATION_HALF_DECIBEL, oversampling.go:13 */

static inline bool gdg_deliver_factor_ok(int factor) { return factor == 1 || factor == 2 || factor == 4; }
/* the taps of the factor's anti-aliasing filter (aa_taps.h): 77 and 155; none at factor 1 */
static inline int gdg_deliver_tap_count(int factor) { return factor == 2 ? 77 : factor == 4 ? 155 : 0; }
/* session samples a delivered port lags the render by: (T - 1) / 2 */
static inline int gdg_deliver_latency(int factor) { return factor == 2 ? 38 : factor == 4 ? 77 : 0; }

/*
 * The ratio stage behind the factor (include/gdg.h, DELIVERY, "a rational ratio"): L / M (up / down) applied to the intermediate rows at
 * rate / R.  Everything here is 64-bit integer arithmetic on job indices; no floating point.
 */
#define GDG_DELIVER_RATIO_HISTORY 127                /* intermediate samples a port keeps from step to step: the longest phase filter's reach, T - 1 of T = 128 */
#define GDG_DELIVER_RATIO_MAX_UP 160
#define GDG_DELIVER_RATIO_MAX_DOWN 320
#define GDG_DELIVER_RATIO_MAX_TAPS 128

static inline unsigned long long gdg_deliver_gcd(unsigned long long a, unsigned long long b) { while (b) { const unsigned long long t = a % b; a = b; b = t; } return a; }
/* admissible: reduced, 1 <= L <= 160, 1 <= M <= 320, M <= 2 L and L <= 2 M; 1 / 1 = no ratio stage */
static inline bool gdg_deliver_ratio_ok(int up, int down) {
    return up >= 1 && up <= GDG_DELIVER_RATIO_MAX_UP && down >= 1 && down <= GDG_DELIVER_RATIO_MAX_DOWN && down <= 2 * up && up <= 2 * down &&
           gdg_deliver_gcd((unsigned long long)up, (unsigned long long)down) == 1;
}
static inline bool gdg_deliver_ratio_on(int up, int down) { return up != 1 || down != 1; }
/* taps per phase: T = 2 * ceil(32 * max(1, M / L)): 64 while M <= L, 70 at 147 / 160, at most 128; 0 without a ratio stage */
static inline int gdg_deliver_ratio_tap_count(int up, int down) {
    if (!gdg_deliver_ratio_ok(up, down) || !gdg_deliver_ratio_on(up, down)) return 0;
    return down <= up ? 64 : 2 * ((32 * down + up - 1) / up);
}
/* session samples a port delivered at factor R and ratio L / M lags the render by: the factor's, and R * T / 2 */
static inline int gdg_deliver_ratio_latency(int factor, int up, int down) {
    if (!gdg_deliver_factor_ok(factor) || !gdg_deliver_ratio_ok(up, down)) return 0;
    return gdg_deliver_latency(factor) + factor * (gdg_deliver_ratio_tap_count(up, down) / 2);
}
/* the first output that does not lie in front of intermediate sample s: ceil(s L / M) */
static inline unsigned long long gdg_deliver_ratio_first(unsigned long long s, int up, int down) {
    return (s * (unsigned long long)up + (unsigned long long)down - 1) / (unsigned long long)down;
}
/* the outputs the intermediate samples [s0, s0 + count) produce: ceil(s0 L / M) <= n < ceil((s0 + count) L / M) */
static inline unsigned long long gdg_deliver_ratio_count(unsigned long long s0, unsigned long long count, int up, int down) {
    return gdg_deliver_ratio_first(s0 + count, up, down) - gdg_deliver_ratio_first(s0, up, down);
}
/* the delivered samples the session samples [first, first + count) produce, both multiples of the factor */
static inline unsigned long long gdg_deliver_samples(int factor, int up, int down, unsigned long long first, unsigned long long count) {
    return gdg_deliver_ratio_count(first / (unsigned long long)factor, count / (unsigned long long)factor, up, down);
}
/* the most delivered samples any `count` session samples produce, wherever they begin, rounded up to the encoders' groups of four: a row's
 * fixed pitch in the scratch rows and what a window's room is made for */
static inline size_t gdg_deliver_pitch(int factor, int up, int down, size_t count) {
    const unsigned long long most = gdg_deliver_ratio_first((unsigned long long)count / (unsigned long long)factor, up, down);      /* ceil(c L / M): a count is that or one less */
    return (size_t)((most + 3) & ~3ull);
}

/* a step of w blocks that begins `off` session samples into its slice: what its rows weigh at factor R and the sample width `width` */
struct DeliverStep {
    size_t samples;        /* delivered samples of a row: w * 8192 / R, with a ratio the count above */
    size_t row_bytes;      /* the pitch of a row in the encoded half and on its way down: `pitch` samples in bytes */
    size_t file_at;        /* where the step's bytes begin in a port's out_bytes buffer: off / R * width, with a ratio (n0 - the slice's n0) * width */
    size_t rows_end;       /* `rows` encoded rows, compact: where whatever rides behind them (a shard's float64 rows from the next 16 bytes on, the record sections) begins */
    size_t pitch;          /* samples a row is encoded with: `samples` rounded up to a multiple of four (the ratio kernel writes +0.0 into the pad) */
    size_t copy_bytes;     /* what the host's scatter copies of each row: samples * width */
    size_t inter_first;    /* the job index of the step's first intermediate sample: (pos + off) / R */
    size_t inter_samples;  /* ... and how many it has: w * 8192 / R */
    size_t first_out;      /* the job index of the step's first delivered sample: the dither's index of sample 0 of its rows */
};
/* ... of a slice that begins at session sample `pos` of its job, with the ratio L / M behind the factor */
static inline DeliverStep deliver_ratio_step(size_t w, size_t off, size_t pos, int R, int L, int M, size_t width, size_t rows) {
    DeliverStep s;
    s.inter_first = (pos + off) / (size_t)R;
    s.inter_samples = w * (size_t)GDG_DELIVER_BLOCK / (size_t)R;
    s.first_out = (size_t)gdg_deliver_ratio_first(s.inter_first, L, M);
    s.samples = (size_t)gdg_deliver_ratio_count(s.inter_first, s.inter_samples, L, M);
    s.pitch = (s.samples + 3) & ~(size_t)3;
    s.row_bytes = s.pitch * width;
    s.copy_bytes = s.samples * width;
    s.file_at = (s.first_out - (size_t)gdg_deliver_ratio_first(pos / (size_t)R, L, M)) * width;
    s.rows_end = rows * s.row_bytes;
    return s;
}
/* ... and without one (1 / 1): the figures of the factor alone, wherever the slice begins */
static inline DeliverStep deliver_step(size_t w, size_t off, int R, size_t width, size_t rows) { return deliver_ratio_step(w, off, 0, R, 1, 1, width, rows); }
/* the download of a step in K pieces of whole rows: piece c begins with row rows * c / K */
static inline size_t deliver_chunk_row(size_t rows, int c, int K) { return rows * (size_t)c / (size_t)K; }
/* ... and covers the bytes [b0, b1) of the half; the last piece takes everything up to `down`, the end of what the step sends */
static inline void deliver_chunk_bytes(size_t rows, size_t row_bytes, int c, int K, size_t down, size_t *b0, size_t *b1) {
    *b0 = deliver_chunk_row(rows, c, K) * row_bytes;
    *b1 = (c + 1 == K) ? down : deliver_chunk_row(rows, c + 1, K) * row_bytes;
}
/* the room a half needs for the encoded rows of a window of W blocks */
static inline size_t deliver_ratio_window_bytes(size_t W, int R, int L, int M, size_t width, size_t rows) { return rows * gdg_deliver_pitch(R, L, M, W * (size_t)GDG_DELIVER_BLOCK) * width; }
static inline size_t deliver_window_bytes(size_t W, int R, size_t width, size_t rows) { return deliver_ratio_window_bytes(W, R, 1, 1, width, rows); }

#endif
