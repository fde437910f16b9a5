/*
 * deliver_kernels.h -- the delivery of finished float64 rows at a half or a quarter of the session rate (include/gdg.h, DELIVERY; deliver.h;
 * DESIGN.md 4.12i).  Included by io.hip, in front of the encoders' callers: a reader of the window's rows like the blends, with a small
 * history per row like theirs.  oversampling.Decimate (oversampling.go:126-184) without the filter's clip: for output i of a row x
 *   f = h[0] x[R i];  f = f + h[k] x[R i - k], k = 1 .. T - 1 ascending;  y[i] = A f
 * every product and every add rounded on its own (__dmul_rn, __dadd_rn: no contraction however this file is compiled), the symmetric taps
 * never folded.  x[n] for n < 0 is the history's (the 154 samples in front of the launch) or +0.0.
 *
 * deliver_rows_kernel<R>: blockIdx.y = the row, blockIdx.x = a tile of DELIVER_T = 256 outputs, a thread per output.
 *   - the tile's R * 256 + T - 1 session samples are read ONCE from global memory, by 16-byte loads where the launcher has seen that rows and
 *     history allow them (VEC; 8-byte loads otherwise, the same values), and staged in LDS.  The window begins at session sample
 *     R * tile - (T - 1): even, so a 16-byte pair lies wholly in the history, in the row or behind its end (samples is a multiple of R).
 *   - the LDS layout is polyphase: window slot m lies at phase m % R, index m / R.  Thread t reads, for tap k, slot R t + (T - 1 - k): at a
 *     fixed k every lane reads the same phase at consecutive indices -- 8 bytes apart, two banks a lane, 64 banks per 32-lane group: no
 *     bank conflict (ds_read_b64 resolves conflicts within each half of the wave), and the offset is an immediate of the unrolled loop.
 *   - the taps come through uniform loads (k is the unrolled loop's constant, the table a kernel argument: scalar loads into SGPRs), as the
 *     oversampler's do; a tap is an SGPR operand of its multiply.
 *   - outputs are stored 8 bytes a lane, 512 bytes a wave, coalesced.
 * LDS: (R * 256 + T - 1 rounded up to R) doubles: 4 704 bytes at R = 2, 9 440 bytes at R = 4.
 *
 * deliver_history_save_kernel: the last 154 of the launch's samples of every row become the next launch's history; when the launch had fewer
 * than 154 the old history moves up in front of them.  One workgroup per row reads its 154 values, meets at a barrier and writes them, so
 * the move is safe in place.
 */
#include "deliver.h"

#define DELIVER_T 256

template <int R> struct deliver_shape {
    static constexpr int T = R == 2 ? 77 : 155;
    static constexpr int WIN = R * DELIVER_T + T - 1;                      /* slots of a tile's window: even */
    static constexpr int PHASE = (WIN + R - 1) / R;                        /* slots per phase */
};

template <int R, bool VEC>
__global__ void __launch_bounds__(DELIVER_T)
deliver_rows_kernel(const double *rows, size_t row_stride, size_t samples, const double *__restrict__ taps, const double *history, double *out, size_t out_stride) {
    using S = deliver_shape<R>;
    constexpr int T = S::T;
    __shared__ double win[R * S::PHASE];
    const double *x = rows + (size_t)blockIdx.y * row_stride;
    const double *hist = history ? history + (size_t)blockIdx.y * GDG_DELIVER_HISTORY : nullptr;
    const size_t n_out = samples / R, o0 = (size_t)blockIdx.x * DELIVER_T;
    const long long base = (long long)(R * o0) - (T - 1);                  /* the session sample of window slot 0 */
    /* the session sample s, from the history in front of the launch, the row, or +0.0 on either side */
    auto sample = [&](long long s) -> double {
        if (s < 0) return (hist && s >= -(long long)GDG_DELIVER_HISTORY) ? hist[GDG_DELIVER_HISTORY + s] : 0.0;
        return s < (long long)samples ? x[s] : 0.0;
    };
    if (VEC) {
        for (int m = 2 * (int)threadIdx.x; m < S::WIN; m += 2 * DELIVER_T) {
            const long long s = base + m;                                   /* even: the pair lies on one side of 0 and of `samples` */
            v2d q = { 0.0, 0.0 };
            if (s < 0) { if (hist && s >= -(long long)GDG_DELIVER_HISTORY) q = *reinterpret_cast<const v2d *>(hist + (GDG_DELIVER_HISTORY + s)); }
            else if (s < (long long)samples) q = *reinterpret_cast<const v2d *>(x + s);
            win[(m % R) * S::PHASE + m / R] = q.x;
            win[((m + 1) % R) * S::PHASE + (m + 1) / R] = q.y;
        }
    } else {
        for (int m = (int)threadIdx.x; m < S::WIN; m += DELIVER_T) win[(m % R) * S::PHASE + m / R] = sample(base + m);
    }
    __syncthreads();
    const size_t o = o0 + threadIdx.x;
    if (o >= n_out) return;
    const double *w = win + threadIdx.x;
    double f = __dmul_rn(taps[0], w[((T - 1) % R) * S::PHASE + (T - 1) / R]);
#pragma unroll
    for (int k = 1; k < T; k++) {
        const int q = T - 1 - k;                                            /* a constant of the unrolled loop: the read's offset is an immediate */
        f = __dadd_rn(f, __dmul_rn(taps[k], w[(q % R) * S::PHASE + q / R]));
    }
    out[(size_t)blockIdx.y * out_stride + o] = __dmul_rn(GDG_DELIVER_ATTENUATION, f);
}

__global__ void __launch_bounds__(DELIVER_T)
deliver_history_save_kernel(const double *rows, size_t row_stride, size_t samples, double *history) {
    const int j = (int)threadIdx.x;
    double *hist = history + (size_t)blockIdx.x * GDG_DELIVER_HISTORY;
    double v = 0.0;
    if (j < GDG_DELIVER_HISTORY) {
        const long long s = (long long)samples - GDG_DELIVER_HISTORY + j;   /* the session sample that becomes entry j */
        v = s >= 0 ? rows[(size_t)blockIdx.x * row_stride + (size_t)s] : hist[GDG_DELIVER_HISTORY + s];
    }
    __syncthreads();
    if (j < GDG_DELIVER_HISTORY) hist[j] = v;
}

/* rows of `samples` session samples (a positive multiple of `factor`, 2 or 4; row r at d_rows + r * row_stride, 8-byte aligned) -> rows of
 * samples / factor delivered samples at d_out + r * out_stride.  d_taps: the factor's expanded table (77 or 155 doubles) in device memory.
 * d_history: null (+0.0 in front of sample 0) or [n_rows][154], read only.  d_out overlaps neither the rows nor the history. */
hipError_t gdg_launch_deliver_rows(int factor, const double *d_rows, size_t row_stride, size_t samples, unsigned n_rows, const double *d_taps, const double *d_history,
                                   double *d_out, size_t out_stride, hipStream_t s) {
    if (n_rows == 0) return hipSuccess;
    if ((factor != 2 && factor != 4) || !d_rows || !d_taps || !d_out || samples == 0 || samples % (size_t)factor || row_stride < samples ||
        out_stride < samples / (size_t)factor || samples / (size_t)factor > (size_t)0x7fffffff * DELIVER_T || ((uintptr_t)d_rows & 7) || ((uintptr_t)d_out & 7) ||
        ((uintptr_t)d_history & 7) || ((uintptr_t)d_taps & 7))
        return hipErrorInvalidValue;
    const size_t n_out = samples / (size_t)factor;
    const bool vec = !((uintptr_t)d_rows & 15) && !(row_stride & 1) && !((uintptr_t)d_history & 15);      /* a history row is 154 doubles: 16-byte aligned with its base */
    for (unsigned r0 = 0; r0 < n_rows; r0 += 65535u) {                      /* gridDim.y holds 65535 rows */
        const unsigned nr = n_rows - r0 < 65535u ? n_rows - r0 : 65535u;
        const dim3 grid((unsigned)((n_out + DELIVER_T - 1) / DELIVER_T), nr);
        const double *rows = d_rows + (size_t)r0 * row_stride, *hist = d_history ? d_history + (size_t)r0 * GDG_DELIVER_HISTORY : nullptr;
        double *out = d_out + (size_t)r0 * out_stride;
        if (factor == 2) {
            if (vec) deliver_rows_kernel<2, true><<<grid, DELIVER_T, 0, s>>>(rows, row_stride, samples, d_taps, hist, out, out_stride);
            else deliver_rows_kernel<2, false><<<grid, DELIVER_T, 0, s>>>(rows, row_stride, samples, d_taps, hist, out, out_stride);
        } else {
            if (vec) deliver_rows_kernel<4, true><<<grid, DELIVER_T, 0, s>>>(rows, row_stride, samples, d_taps, hist, out, out_stride);
            else deliver_rows_kernel<4, false><<<grid, DELIVER_T, 0, s>>>(rows, row_stride, samples, d_taps, hist, out, out_stride);
        }
    }
    return hipGetLastError();
}

/* behind the launch above and before anything writes the rows again: d_history[n_rows][154] takes the rows' last 154 samples */
hipError_t gdg_launch_deliver_history_save(const double *d_rows, size_t row_stride, size_t samples, unsigned n_rows, double *d_history, hipStream_t s) {
    if (n_rows == 0) return hipSuccess;
    if (!d_rows || !d_history || samples == 0 || row_stride < samples || ((uintptr_t)d_rows & 7) || ((uintptr_t)d_history & 7)) return hipErrorInvalidValue;
    deliver_history_save_kernel<<<n_rows, DELIVER_T, 0, s>>>(d_rows, row_stride, samples, d_history);
    return hipGetLastError();
}
