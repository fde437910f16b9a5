/*
 * dither.h -- TPDF dither with rounding for the four LPCM encoders (gdg_batch_set_dither, include/gdg.h states the arithmetic): the hash,
 * the key of a port, the noise of a sample and the quantiser as __host__ __device__ inlines -- the encoder kernels of io.hip use them, and
 * so can a stand-alone host program (tests/native/dither_check.cpp) -- and the pure host arithmetic behind the configuration: which port a
 * row of a launch is, the range check of port_base + n, the master cursor's overflow.  No HIP header is needed to compile this file.
 */
#ifndef GDG_DITHER_H
#define GDG_DITHER_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GDG_DITHER_HD __host__ __device__ __forceinline__
#else
#define GDG_DITHER_HD static inline
#endif

/* the constants of the checkpoint digest (include/gdg.h; gdg_internal.h: GDG_DIGEST_K, _M0, _M1) */
#define GDG_DITHER_K  0x9e3779b97f4a7c15ull
#define GDG_DITHER_M0 0xff51afd7ed558ccdull
#define GDG_DITHER_M1 0xc4ceb9fe1a85ec53ull

/* the job-wide outputs have fixed ports: a shard need not know the job's channel count */
#define GDG_DITHER_PORT_MASTER_LEFT  0xfffffffdu
#define GDG_DITHER_PORT_MASTER_RIGHT 0xfffffffeu
#define GDG_DITHER_PORT_METRONOME    0xffffffffu

/* the four LPCM formats are enum gdg_wave_format 0 .. 3 (LPCM8, 16, 24, 32); IEEE32 and IEEE64 are never dithered */
GDG_DITHER_HD bool gdg_dither_applies(int mode, int fmt) { return mode == 1 && fmt >= 0 && fmt <= 3; }

/* every product and every add of the quantiser is rounded on its own: never a fused multiply-add, on any compiler */
#if defined(__HIP_DEVICE_COMPILE__)
#define GDG_DITHER_MUL(a, b) __dmul_rn((a), (b))
#define GDG_DITHER_ADD(a, b) __dadd_rn((a), (b))
#else
static inline double gdg_dither_mul_(double a, double b) { volatile double r = a * b; return r; }
static inline double gdg_dither_add_(double a, double b) { volatile double r = a + b; return r; }
#define GDG_DITHER_MUL(a, b) gdg_dither_mul_((a), (b))
#define GDG_DITHER_ADD(a, b) gdg_dither_add_((a), (b))
#endif

GDG_DITHER_HD uint64_t gdg_dither_fmix(uint64_t x) {
    x ^= x >> 33;
    x *= GDG_DITHER_M0;
    x ^= x >> 33;
    x *= GDG_DITHER_M1;
    return x ^ (x >> 33);
}

/* once per row */
GDG_DITHER_HD uint64_t gdg_dither_key(uint64_t seed, uint32_t port) { return gdg_dither_fmix(seed + ((uint64_t)port + 1u) * GDG_DITHER_K); }

/* one hash per sample yields both 32-bit words */
GDG_DITHER_HD uint64_t gdg_dither_hash(uint64_t key, uint64_t index) { return gdg_dither_fmix((index + GDG_DITHER_K) ^ key); }

/* triangular on (-1, 1) codes; the difference of two 32-bit words has 33 bits: exact in float64 */
GDG_DITHER_HD double gdg_dither_noise(uint64_t h) {
    const int64_t a = (int64_t)(h >> 32), b = (int64_t)(h & 0xffffffffull);
    return (double)(a - b) * (1.0 / 4294967296.0);
}

/* the signed code of sample x with noise d: floor((S clamp1(x) + d) + 0.5), clamped to the format's range */
GDG_DITHER_HD long long gdg_dither_quantise(int fmt, double x, double d) {
    const double S = fmt == 0 ? 127.0 : fmt == 1 ? 32767.5 : fmt == 2 ? 8388607.5 : 2147483647.5;      /* the plain encoder's constants */
    const double hi = fmt == 0 ? 127.0 : fmt == 1 ? 32767.0 : fmt == 2 ? 8388607.0 : 2147483647.0, lo = -hi - 1.0;
    x = x < -1.0 ? -1.0 : (x > 1.0 ? 1.0 : x);
    double q = floor(GDG_DITHER_ADD(GDG_DITHER_ADD(GDG_DITHER_MUL(S, x), d), 0.5));
    q = q < lo ? lo : (q > hi ? hi : q);
    return (long long)q;
}

/* ... and the sample's little-endian bytes as the plain encoder of io.hip returns them (LPCM8: + 128 afterwards, 0 .. 255) */
GDG_DITHER_HD unsigned gdg_dither_code(int fmt, double x, uint64_t key, uint64_t index) {
    const long long q = gdg_dither_quantise(fmt, x, gdg_dither_noise(gdg_dither_hash(key, index)));
    if (fmt == 0) { const long long r = q + 128; return (unsigned)(r < 0 ? 0 : (r > 255 ? 255 : r)); }
    if (fmt == 1) return (unsigned)q & 0xffffu;
    if (fmt == 2) return (unsigned)q & 0xffffffu;
    return (unsigned)(int)q;
}

/* ---- the configuration's arithmetic (host and device alike) ---------------------------------------------------------------------------- */
/* A launch encodes `n_chain` chain rows whose ports start at port_base, then the job-wide rows in the files' order: master left, master
 * right, metronome.  (A shard's metronome track alone: one "chain" row at GDG_DITHER_PORT_METRONOME.) */
GDG_DITHER_HD uint32_t gdg_dither_row_port(uint32_t port_base, uint32_t n_chain, uint32_t row) {
    return row < n_chain ? port_base + row : GDG_DITHER_PORT_MASTER_LEFT + (row - n_chain);
}

/* the chain ports [port_base, port_base + n_channels) stay below the fixed ones */
GDG_DITHER_HD bool gdg_dither_ports_ok(uint32_t port_base, int n_channels) {
    return n_channels >= 0 && (uint64_t)port_base + (uint64_t)n_channels < (uint64_t)GDG_DITHER_PORT_MASTER_LEFT;
}

/* the master cursor behind a slice of `samples`: false when it would pass 2^64 (*next is then left alone) */
GDG_DITHER_HD bool gdg_dither_advance(uint64_t cursor, uint64_t samples, uint64_t *next) {
    if (samples > ~(uint64_t)0 - cursor) return false;
    *next = cursor + samples;
    return true;
}

#endif
