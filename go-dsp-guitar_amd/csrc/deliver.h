/*
 * deliver.h -- the delivery of batch outputs at a half or a quarter of the session rate (include/gdg.h, DELIVERY): the factor's rules and the
 * ONE statement of the byte counts of a delivered step.  Every port that leaves the device encoded has samples / R samples, so whatever a
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

/* a step of w blocks that begins `off` session samples into its slice: what its rows weigh at factor R and the sample width `width` */
struct DeliverStep {
    size_t samples;        /* delivered samples of a row: w * 8192 / R */
    size_t row_bytes;      /* ... in bytes */
    size_t file_at;        /* where the step's bytes begin in a port's out_bytes buffer: off / R * width */
    size_t rows_end;       /* `rows` encoded rows, compact: where whatever rides behind them (a shard's float64 rows from the next 16 bytes on, the record sections) begins */
};
static inline DeliverStep deliver_step(size_t w, size_t off, int R, size_t width, size_t rows) {
    DeliverStep s;
    s.samples = w * (size_t)GDG_DELIVER_BLOCK / (size_t)R;
    s.row_bytes = s.samples * width;
    s.file_at = off / (size_t)R * width;
    s.rows_end = rows * s.row_bytes;
    return s;
}
/* the download of a step in K pieces of whole rows: piece c begins with row rows * c / K */
static inline size_t deliver_chunk_row(size_t rows, int c, int K) { return rows * (size_t)c / (size_t)K; }
/* ... and covers the bytes [b0, b1) of the half; the last piece takes everything up to `down`, the end of what the step sends */
static inline void deliver_chunk_bytes(size_t rows, size_t row_bytes, int c, int K, size_t down, size_t *b0, size_t *b1) {
    *b0 = deliver_chunk_row(rows, c, K) * row_bytes;
    *b1 = (c + 1 == K) ? down : deliver_chunk_row(rows, c + 1, K) * row_bytes;
}
/* the room a half needs for the encoded rows of a window of W blocks */
static inline size_t deliver_window_bytes(size_t W, int R, size_t width, size_t rows) { return rows * (W * (size_t)GDG_DELIVER_BLOCK / (size_t)R) * width; }

#endif
