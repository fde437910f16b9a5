/*
 * deliver_ratio_kernels.h -- the ratio stage of the delivery (include/gdg.h, DELIVERY, "a rational ratio"; deliver.h): the
 * intermediate rows at rate / R resampled by L / M in front of the untouched encoders.  Included by io.hip behind deliver_kernels.h.  For
 * output n of a row x over the whole job, b = floor(n M / L), p = (n M) mod L:
 *   f = tap[p][0] x[b];  f = f + tap[p][t] x[b - t], t = 1 .. T - 1 ascending;  y[n] = f
 * every product and every add rounded on its own (__dmul_rn, __dadd_rn), no attenuation, no clip.  x[k] in front of the launch is the
 * history's (the 127 intermediate samples in front of it) or +0.0.
 *
 * deliver_ratio_kernel: blockIdx.y = the row, blockIdx.x = a tile of DELIVER_T = 256 consecutive outputs, a thread per output.
 *   - indices: the launcher hands over n0 = ceil(first L / M), the job index of the launch's first output.  The tile's first output has
 *     n0 + 256 tile; its n M is split ONCE per workgroup into q0 = (n M) / L and r0 = (n M) % L in 64 bits (uniform: scalar code); a lane
 *     adds lane * M to r0 -- below 160 + 255 * 320, 32 bits -- and has b = q0 + v / L, p = v % L.
 *   - the tile's intermediate samples, job indices q0 - (T - 1) .. b of its last lane -- at most 255 M / L + 1 + T - 1 <= 638 -- are read ONCE
 *     and staged in LDS, linear.  The window begins at an even offset into the row (one slot more: 639 of 640), so that with `vec` a pair of
 *     slots is one 16-byte load wherever both lie in the row (`vec`: the launcher has seen that the rows allow it); slots in front of the row (the history) and the last one of an odd row are
 *     8-byte loads.  Behind the launch's last sample nothing is needed (the filter is causal) and +0.0 is staged.
 *   - the lanes of a tile have different phases, so the taps cannot be uniform operands as deliver_rows_kernel's are.  They come from a
 *     [T][L] copy of the table in device memory: at a fixed t the 64 lanes of a wave read tapT[t L + p] inside one run of 8 L <= 1280 bytes,
 *     which the vector cache serves from a few lines; consecutive t walk consecutive runs.  (The [L][T] form would spread a wave's load at
 *     a fixed t over 64 rows 8 T bytes apart: 64 lines per load.)
 *   - lane l reads slot b_l - t: neighbours are M / L slots apart -- 0.5 to 2 -- so a ds_read_b64 of a 32-lane half touches at most 64
 *     slots = 2 bank rows: two-way at M = 2 L, free at M <= L.
 *   - outputs are stored 8 bytes a lane, coalesced; lanes in [n_out, n_pad) store +0.0: the pad up to the encoders' group of four.
 * LDS: 640 doubles = 5 120 bytes.
 *
 * deliver_ratio_history_save_kernel: deliver_history_save_kernel for the 127 intermediate samples.
 */
#include "deliver.h"

#define DELIVER_RATIO_WIN 640

struct gdg_deliver_ratio_launch {
    int L, M, T;
    unsigned long long n0;          /* job index of the launch's first output: ceil(first L / M) */
    unsigned long long first;       /* job index of the launch's first intermediate sample */
    unsigned long long n_out;       /* outputs of a row */
    unsigned long long n_pad;       /* ... and with the +0.0 behind them: n_out <= n_pad <= out_stride */
};

/* Both kernels of this file have C linkage: tests/test_deliver_host.py takes its census of io.hip's delivery kernels by their C++-mangled names
 * and holds it at the factor stage's five, so these two go by their plain names (tests/test_deliver_ratio_abi.py holds them by those).  One
 * text for both load paths: `vec` is uniform, and the branch on it is the staging loop's only cost. */
extern "C" __global__ void __launch_bounds__(DELIVER_T)
deliver_ratio_kernel(const double *rows, size_t row_stride, size_t samples, gdg_deliver_ratio_launch a, const double *__restrict__ tapsT, const double *history, double *out,
                     size_t out_stride, int vec) {
    __shared__ double win[DELIVER_RATIO_WIN];
    const double *x = rows + (size_t)blockIdx.y * row_stride;
    const double *hist = history ? history + (size_t)blockIdx.y * GDG_DELIVER_RATIO_HISTORY : nullptr;
    const int L = a.L, M = a.M, T = a.T;
    const unsigned long long j0 = (unsigned long long)blockIdx.x * DELIVER_T;      /* the tile's first output, counted in the launch */
    const unsigned long long nm = (a.n0 + j0) * (unsigned long long)M;
    const unsigned long long q0 = nm / (unsigned long long)L;
    const unsigned r0 = (unsigned)(nm % (unsigned long long)L);
    /* slot 0: the intermediate sample q0 - (T - 1), as an offset into the row, down to the even one below */
    const long long base = ((long long)(q0 - a.first) - (T - 1)) & ~1ll;
    const unsigned long long left = a.n_out - j0 < DELIVER_T ? a.n_out - j0 : DELIVER_T;      /* the tile's outputs (the launcher makes no tile behind n_pad; left may be 0 in the pad's) */
    const int need = a.n_out > j0 ? (int)((long long)(q0 - a.first) + (long long)((r0 + (unsigned)(left - 1) * (unsigned)M) / (unsigned)L) - base) + 1 : 0;
    auto sample = [&](long long s) -> double {
        if (s < 0) return (hist && s >= -(long long)GDG_DELIVER_RATIO_HISTORY) ? hist[GDG_DELIVER_RATIO_HISTORY + s] : 0.0;
        return s < (long long)samples ? x[s] : 0.0;
    };
    if (vec) {
        for (int m = 2 * (int)threadIdx.x; m < need; m += 2 * DELIVER_T) {
            const long long s = base + m;                                   /* even */
            if (s >= 0 && s + 1 < (long long)samples) {
                const v2d q = *reinterpret_cast<const v2d *>(x + s);
                win[m] = q.x;
                win[m + 1] = q.y;
            } else {
                win[m] = sample(s);
                win[m + 1] = sample(s + 1);
            }
        }
    } else {
        for (int m = (int)threadIdx.x; m < need; m += DELIVER_T) win[m] = sample(base + m);
    }
    __syncthreads();
    const unsigned long long j = j0 + threadIdx.x;
    if (j >= a.n_pad) return;
    double *y = out + (size_t)blockIdx.y * out_stride + j;
    if (j >= a.n_out) { *y = 0.0; return; }
    const unsigned v = r0 + threadIdx.x * (unsigned)M;
    const unsigned p = v % (unsigned)L;
    const double *w = win + ((long long)(q0 - a.first) + (long long)(v / (unsigned)L) - base);      /* the slot of x[b] */
    const double *h = tapsT + p;
    double f = __dmul_rn(h[0], w[0]);
#pragma unroll 4
    for (int t = 1; t < T; t++) f = __dadd_rn(f, __dmul_rn(h[(size_t)t * (size_t)L], w[-t]));
    *y = f;
}

extern "C" __global__ void __launch_bounds__(DELIVER_T)
deliver_ratio_history_save_kernel(const double *rows, size_t row_stride, size_t samples, double *history) {
    const int j = (int)threadIdx.x;
    double *hist = history + (size_t)blockIdx.x * GDG_DELIVER_RATIO_HISTORY;
    double v = 0.0;
    if (j < GDG_DELIVER_RATIO_HISTORY) {
        const long long s = (long long)samples - GDG_DELIVER_RATIO_HISTORY + j;   /* the launch's sample that becomes entry j */
        v = s >= 0 ? rows[(size_t)blockIdx.x * row_stride + (size_t)s] : hist[GDG_DELIVER_RATIO_HISTORY + s];
    }
    __syncthreads();
    if (j < GDG_DELIVER_RATIO_HISTORY) hist[j] = v;
}

/* rows of `samples` intermediate samples, the job's [first, first + samples) (row r at d_rows + r * row_stride, 8-byte aligned) -> the outputs
 * ceil(first L / M) <= n < ceil((first + samples) L / M) of every row at d_out + r * out_stride, and +0.0 behind them up to `pad_to` samples
 * (0: no pad; otherwise pad_to >= the count and <= out_stride).  d_tapsT: the ratio's table as [T][L] in device memory.  d_history: null
 * (+0.0 in front of the launch) or [n_rows][127], read only.  d_out overlaps neither the rows nor the history.  A launch without an output
 * (a few samples at L < M) writes only the pad. */
hipError_t gdg_launch_deliver_ratio(int up, int down, const double *d_rows, size_t row_stride, size_t samples, unsigned long long first, unsigned n_rows, const double *d_tapsT,
                                    const double *d_history, double *d_out, size_t out_stride, size_t pad_to, hipStream_t s) {
    if (n_rows == 0) return hipSuccess;
    const int T = gdg_deliver_ratio_tap_count(up, down);
    if (!T || !d_rows || !d_tapsT || !d_out || samples == 0 || row_stride < samples || first > (1ull << 48) || samples > (1ull << 40) || ((uintptr_t)d_rows & 7) ||
        ((uintptr_t)d_out & 7) || ((uintptr_t)d_history & 7) || ((uintptr_t)d_tapsT & 7))
        return hipErrorInvalidValue;
    gdg_deliver_ratio_launch a;
    a.L = up; a.M = down; a.T = T;
    a.first = first;
    a.n0 = gdg_deliver_ratio_first(first, up, down);
    a.n_out = gdg_deliver_ratio_count(first, samples, up, down);
    a.n_pad = pad_to > a.n_out ? pad_to : a.n_out;
    if (a.n_pad > out_stride || a.n_pad > (size_t)0x7fffffff * DELIVER_T) return hipErrorInvalidValue;
    if (a.n_pad == 0) return hipSuccess;
    const bool vec = !((uintptr_t)d_rows & 15) && !(row_stride & 1);
    for (unsigned r0 = 0; r0 < n_rows; r0 += 65535u) {                      /* gridDim.y holds 65535 rows */
        const unsigned nr = n_rows - r0 < 65535u ? n_rows - r0 : 65535u;
        const dim3 grid((unsigned)((a.n_pad + DELIVER_T - 1) / DELIVER_T), nr);
        const double *rows = d_rows + (size_t)r0 * row_stride, *hist = d_history ? d_history + (size_t)r0 * GDG_DELIVER_RATIO_HISTORY : nullptr;
        double *out = d_out + (size_t)r0 * out_stride;
        deliver_ratio_kernel<<<grid, DELIVER_T, 0, s>>>(rows, row_stride, samples, a, d_tapsT, hist, out, out_stride, vec ? 1 : 0);
    }
    return hipGetLastError();
}

/* behind the launch above and before anything writes the rows again: d_history[n_rows][127] takes the rows' last 127 samples */
hipError_t gdg_launch_deliver_ratio_history_save(const double *d_rows, size_t row_stride, size_t samples, unsigned n_rows, double *d_history, hipStream_t s) {
    if (n_rows == 0) return hipSuccess;
    if (!d_rows || !d_history || samples == 0 || row_stride < samples || ((uintptr_t)d_rows & 7) || ((uintptr_t)d_history & 7)) return hipErrorInvalidValue;
    deliver_ratio_history_save_kernel<<<n_rows, DELIVER_T, 0, s>>>(d_rows, row_stride, samples, d_history);
    return hipGetLastError();
}
