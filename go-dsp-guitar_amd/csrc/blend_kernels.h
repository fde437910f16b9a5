/*
 * blend_kernels.h -- the blend outputs (include/gdg.h, gdg_batch_set_blends and gdg_blend_rows): row b of
 * `out` is the weighted sum of blend b's terms over the rows of `rows`, s = w_0 x[c_0] and then s = s + w_k x[c_k] in term order, every
 * product and every add rounded on its own (blend.h).  Three kernels -- plain terms, delayed terms, filtered terms -- behind ONE launcher,
 * gdg_launch_blend at the end of this file, which takes the table as a gdg_blend_view and picks the kernel by what the view holds; the plain
 * and the delayed kernel share one term loop (blend_terms) and differ in how a term is loaded.  No reference counterpart; included by io.hip
 * next to the record kernels and compiled like them without contraction.
 *
 * The plain kernel:
 * blockIdx.y = the blend, blockIdx.x covers the live width.  A lane takes one 16-byte pair of samples where the launcher has seen that every
 * row of both sides starts 16-byte aligned (VEC), one 8-byte sample otherwise; a VEC launch's last lane takes the odd sample of an odd
 * width by the 8-byte path.  A lane reads and writes only inside [0, samples) of a row.  The term table -- first, channel, weight -- is
 * read at addresses that depend on blockIdx.y alone: uniform, fetched by scalar loads.  The term loop is unrolled by four: four row loads
 * are in flight before the first of their adds, and the adds stay in term order.  No LDS, no atomics, no scratch, and plain loads and stores
 * on both sides: the chain rows are read again by the encoder, the blend rows at once by the encoder and the record kernels.
 */
#define BLEND_T 256

template <typename T> struct blend_ops;
template <> struct blend_ops<double> {
    static __device__ __forceinline__ double mul(double w, double x) { return gdg_blend_mul(w, x); }
    static __device__ __forceinline__ double add(double s, double p) { return gdg_blend_add(s, p); }
};
template <> struct blend_ops<v2d> {
    static __device__ __forceinline__ v2d mul(double w, v2d x) { const v2d r = { gdg_blend_mul(w, x.x), gdg_blend_mul(w, x.y) }; return r; }
    static __device__ __forceinline__ v2d add(v2d s, v2d p) { const v2d r = { gdg_blend_add(s.x, p.x), gdg_blend_add(s.y, p.y) }; return r; }
};

/* the terms [k0, k1) at sample `at` (T = v2d: the pair at, at + 1); load(k): term k's sample or pair */
template <typename T, typename Load>
__device__ __forceinline__ void blend_terms(size_t at, const double *__restrict__ weight, int k0, int k1, double *dst, Load load) {
    typedef blend_ops<T> op;
    int k = k0;
    T s = op::mul(weight[k], load(k));
    k++;
    for (; k + 4 <= k1; k += 4) {
        const T x0 = load(k), x1 = load(k + 1), x2 = load(k + 2), x3 = load(k + 3);
        s = op::add(s, op::mul(weight[k], x0));
        s = op::add(s, op::mul(weight[k + 1], x1));
        s = op::add(s, op::mul(weight[k + 2], x2));
        s = op::add(s, op::mul(weight[k + 3], x3));
    }
    for (; k < k1; k++) s = op::add(s, op::mul(weight[k], load(k)));
    *reinterpret_cast<T *>(dst + at) = s;
}

/* plain terms: sample `at` of row channel[k] */
template <typename T>
__device__ __forceinline__ void blend_row_terms(const double *rows, size_t row_stride, size_t at, const int *__restrict__ channel, const double *__restrict__ weight,
                                                int k0, int k1, double *dst) {
    blend_terms<T>(at, weight, k0, k1, dst, [&](int k) { return *reinterpret_cast<const T *>(rows + (size_t)channel[k] * row_stride + at); });
}

template <bool VEC>
__global__ void __launch_bounds__(BLEND_T)
blend_rows_kernel(const double *rows, size_t row_stride, size_t samples, const int *__restrict__ first, const int *__restrict__ channel,
                  const double *__restrict__ weight, double *out, size_t out_stride) {
    const int k0 = first[blockIdx.y], k1 = first[blockIdx.y + 1];
    double *dst = out + (size_t)blockIdx.y * out_stride;
    const size_t at = ((size_t)blockIdx.x * BLEND_T + threadIdx.x) * (VEC ? 2 : 1);
    if (at >= samples) return;
    if (VEC && at + 1 < samples) blend_row_terms<v2d>(rows, row_stride, at, channel, weight, k0, k1, dst);
    else blend_row_terms<double>(rows, row_stride, at, channel, weight, k0, k1, dst);
}

/*
 * Delayed terms (include/gdg.h, BLEND: x_k[i] = x[c_k][i - d_k]).  The same grid, the same table through scalar loads --
 * now with one delay per term --, the same unroll and the same 16-byte store.  What differs is the load of a term:
 *   - a pair of samples at i - d is 16-byte aligned only when d is even (i is, and so are the row's base and stride in a VEC launch): an
 *     even d loads the pair, an odd d two 8-byte samples.  d comes from the table, so the choice is uniform over the workgroup.
 *   - samples in front of the launch's first come from the history: GDG_BLEND_MAX_DELAY doubles per row, the last of them sample -1, or
 *     +0.0 where the caller has none.  Whether a lane can meet them is decided per TILE: GDG_BLEND_MAX_DELAY is a multiple of a tile's
 *     width, so a tile that starts at or behind it never does and runs the path without the compare (HIST = false); only the first
 *     GDG_BLEND_MAX_DELAY samples of a launch run the other.
 * A load address is formed only after the compare that chose its side: rows are read inside [0, samples), the history inside its run.
 */
static_assert(GDG_BLEND_MAX_DELAY % (2 * BLEND_T) == 0, "a tile lies wholly in front of or wholly behind GDG_BLEND_MAX_DELAY");

/* sample `at` - d of row c (at < samples) */
template <bool HIST>
__device__ __forceinline__ double blend_delayed_one(const double *rows, size_t row_stride, const double *history, size_t hist_stride, int c, size_t at, int d) {
    if (!HIST || at >= (size_t)d) return rows[(size_t)c * row_stride + (at - (size_t)d)];
    return history ? history[(size_t)c * hist_stride + ((size_t)GDG_BLEND_MAX_DELAY + at - (size_t)d)] : 0.0;
}

template <typename T, bool HIST> struct blend_delayed_load;
template <bool HIST> struct blend_delayed_load<double, HIST> {
    static __device__ __forceinline__ double at(const double *rows, size_t row_stride, const double *history, size_t hist_stride, int c, size_t i, int d) {
        return blend_delayed_one<HIST>(rows, row_stride, history, hist_stride, c, i, d);
    }
};
template <bool HIST> struct blend_delayed_load<v2d, HIST> {
    /* i is even and i + 1 < samples; an even d keeps i - d even, and both samples lie on one side of sample 0 */
    static __device__ __forceinline__ v2d at(const double *rows, size_t row_stride, const double *history, size_t hist_stride, int c, size_t i, int d) {
        if (!(d & 1)) {
            if (!HIST || i >= (size_t)d) return *reinterpret_cast<const v2d *>(rows + (size_t)c * row_stride + (i - (size_t)d));
            if (history) return *reinterpret_cast<const v2d *>(history + (size_t)c * hist_stride + ((size_t)GDG_BLEND_MAX_DELAY + i - (size_t)d));
            const v2d z = { 0.0, 0.0 };
            return z;
        }
        const v2d r = { blend_delayed_one<HIST>(rows, row_stride, history, hist_stride, c, i, d),
                        blend_delayed_one<HIST>(rows, row_stride, history, hist_stride, c, i + 1, d) };
        return r;
    }
};

/* delayed terms: sample `at` - delay[k] of row channel[k] */
template <typename T, bool HIST>
__device__ __forceinline__ void blend_delayed_terms(const double *rows, size_t row_stride, const double *history, size_t hist_stride, size_t at,
                                                    const int *__restrict__ channel, const double *__restrict__ weight, const int *__restrict__ delay, int k0, int k1,
                                                    double *dst) {
    blend_terms<T>(at, weight, k0, k1, dst, [&](int k) { return blend_delayed_load<T, HIST>::at(rows, row_stride, history, hist_stride, channel[k], at, delay[k]); });
}

template <bool VEC>
__global__ void __launch_bounds__(BLEND_T)
blend_delayed_kernel(const double *rows, size_t row_stride, size_t samples, const int *__restrict__ first, const int *__restrict__ channel,
                     const double *__restrict__ weight, const int *__restrict__ delay, const double *history, size_t hist_stride, double *out, size_t out_stride) {
    const int k0 = first[blockIdx.y], k1 = first[blockIdx.y + 1];
    double *dst = out + (size_t)blockIdx.y * out_stride;
    const size_t tile = (size_t)blockIdx.x * BLEND_T * (VEC ? 2 : 1), at = tile + (size_t)threadIdx.x * (VEC ? 2 : 1);
    if (at >= samples) return;
    const bool pair = VEC && at + 1 < samples;
    if (tile >= (size_t)GDG_BLEND_MAX_DELAY) {                               /* uniform: no sample of this tile lies in front of the launch */
        if (pair) blend_delayed_terms<v2d, false>(rows, row_stride, history, hist_stride, at, channel, weight, delay, k0, k1, dst);
        else blend_delayed_terms<double, false>(rows, row_stride, history, hist_stride, at, channel, weight, delay, k0, k1, dst);
    } else {
        if (pair) blend_delayed_terms<v2d, true>(rows, row_stride, history, hist_stride, at, channel, weight, delay, k0, k1, dst);
        else blend_delayed_terms<double, true>(rows, row_stride, history, hist_stride, at, channel, weight, delay, k0, k1, dst);
    }
}

/* The history of the next launch: the last GDG_BLEND_MAX_DELAY of `samples` samples of rows 0 .. n_rows - 1 go to d_history[r][GDG_BLEND_MAX_DELAY],
 * so that its last entry is the rows' last sample.  blockIdx.y = the row; a lane moves 16 bytes where both sides allow it, 8 otherwise. */
template <bool VEC>
__global__ void __launch_bounds__(BLEND_T)
blend_history_save_kernel(const double *rows, size_t row_stride, size_t samples, double *history) {
    const size_t at = ((size_t)blockIdx.x * BLEND_T + threadIdx.x) * (VEC ? 2 : 1);
    if (at >= (size_t)GDG_BLEND_MAX_DELAY) return;
    const double *src = rows + (size_t)blockIdx.y * row_stride + (samples - (size_t)GDG_BLEND_MAX_DELAY) + at;
    double *dst = history + (size_t)blockIdx.y * GDG_BLEND_MAX_DELAY + at;
    if (VEC) *reinterpret_cast<v2d *>(dst) = *reinterpret_cast<const v2d *>(src);
    else *dst = *src;
}

/* samples >= GDG_BLEND_MAX_DELAY (a batch step is a whole number of blocks of 8192); d_history overlaps no row */
hipError_t gdg_launch_blend_history_save(const double *d_rows, size_t row_stride, size_t samples, unsigned n_rows, double *d_history, hipStream_t s) {
    if (n_rows == 0) return hipSuccess;
    if (!d_rows || !d_history || samples < (size_t)GDG_BLEND_MAX_DELAY || row_stride < samples || n_rows > 65535u || ((uintptr_t)d_rows & 7) || ((uintptr_t)d_history & 7))
        return hipErrorInvalidValue;
    const bool vec = !((uintptr_t)d_rows & 15) && !(row_stride & 1) && !(samples & 1) && !((uintptr_t)d_history & 15);
    const unsigned lanes = GDG_BLEND_MAX_DELAY / (vec ? 2 : 1);
    const dim3 grid((lanes + BLEND_T - 1) / BLEND_T, n_rows);
    if (vec) blend_history_save_kernel<true><<<grid, BLEND_T, 0, s>>>(d_rows, row_stride, samples, d_history);
    else blend_history_save_kernel<false><<<grid, BLEND_T, 0, s>>>(d_rows, row_stride, samples, d_history);
    return hipGetLastError();
}

/*
 * Filtered terms (include/gdg.h, FILTERS: x_k[i] = h_k[0] x[c_k][i - d_k], then + h_k[t] x[c_k][i - d_k - t] in ascending t; DESIGN.md
 * 4.12f).  The grid and the tiles of blend_delayed_kernel, the table through scalar loads -- now with tap_first and the taps --, the same
 * 16-byte store.  What is new is arithmetic: up to 32 terms x 64 taps per output sample, so a row sample is fetched from global memory once
 * per term and tile, not once per tap:
 *   - a term's WINDOW -- the tile's samples i - d_k and BLEND_F_HALO = 64 samples in front of them, of which the T_k - 1 nearest are read --
 *     is staged in LDS by 8-byte loads, every lane BLEND_F_ROUNDS of them; a slot nothing fills holds +0.0, which is also what lies in front
 *     of a job without a history.  The window's slot m is sample tile - d_k - 64 + m of the row.
 *   - two windows: while the lanes run term k's taps out of one, the loads of term k + 1 are in flight in registers and go into the other
 *     behind the arithmetic; one barrier per term.
 *   - a 16-byte lane owns the outputs l, l + 1 (l even) and slides over the window in aligned pairs A_e = slots (64 + l - e, 65 + l - e), e
 *     even: tap t reads slot 64 + l - t for the first output and 65 + l - t for the second, so an even tap takes A_t and an odd tap the halves
 *     A_{t+1}.y and A_{t-1}.x -- one 16-byte LDS read per two taps, lanes 16 bytes apart.  Each output's taps stay in ascending order.
 *   - a term without taps skips the window: the plain delayed load of blend_delayed_kernel, held in registers over the barrier.
 * Whether a slot can lie in front of the launch is decided per tile as before: a term reaches at most GDG_BLEND_MAX_DELAY samples back, so a
 * tile that starts at or behind it runs the path without the compare.  An address is formed only behind the compare that chose its side:
 * rows are read inside [0, samples), the history inside its run (slot m >= 65 - T_k lies at most d_k + T_k - 1 <= 4096 samples back).
 * No lane leaves before the last barrier; a lane past the width fetches its share of the windows and stores nothing.
 * LDS: 2 windows x (tile + 64) doubles -- 9216 bytes with 16-byte lanes (tile 512), 5120 with 8-byte lanes (tile 256).  No scratch, no atomics.
 */
#define BLEND_F_HALO 64
static_assert(BLEND_F_HALO >= GDG_BLEND_MAX_TAPS && BLEND_F_HALO % 2 == 0, "the halo holds the taps behind the first and keeps pairs aligned");

template <bool VEC> struct blend_filtered_shape {
    static constexpr int PER = VEC ? 2 : 1, TILE = BLEND_T * PER, WIN = TILE + BLEND_F_HALO, ROUNDS = (WIN + BLEND_T - 1) / BLEND_T;
};

/* this lane's share of term (c, d, T)'s window over the tile at `tile`, T >= 1: slot r * BLEND_T + threadIdx.x in x[r] */
template <bool VEC, bool HIST>
__device__ __forceinline__ void blend_filtered_fetch(const double *rows, size_t row_stride, size_t samples, const double *history, size_t hist_stride, int c, int d,
                                                     int T, size_t tile, double (&x)[blend_filtered_shape<VEC>::ROUNDS]) {
    typedef blend_filtered_shape<VEC> S;
#pragma unroll
    for (int r = 0; r < S::ROUNDS; r++) {
        const int m = r * BLEND_T + (int)threadIdx.x;
        x[r] = 0.0;
        if (m >= S::WIN || m < BLEND_F_HALO + 1 - T) continue;
        const size_t to = tile + (size_t)m, back = (size_t)d + BLEND_F_HALO;        /* the slot is sample to - back */
        if (!HIST || to >= back) {
            if (to - back < samples) x[r] = rows[(size_t)c * row_stride + (to - back)];
        } else if (history) {
            x[r] = history[(size_t)c * hist_stride + ((size_t)GDG_BLEND_MAX_DELAY + to - back)];
        }
    }
}

template <bool VEC, bool HIST>
__device__ __forceinline__ void blend_filtered_tile(const double *rows, size_t row_stride, size_t samples, const int *__restrict__ channel,
                                                    const double *__restrict__ weight, const int *__restrict__ delay, const int *__restrict__ tap_first,
                                                    const double *__restrict__ tap, const double *history, size_t hist_stride, int k0, int k1, size_t tile,
                                                    double *dst, double (*win)[blend_filtered_shape<VEC>::WIN]) {
    typedef blend_filtered_shape<VEC> S;
    const int l = (int)threadIdx.x * S::PER;
    const size_t at = tile + (size_t)l;
    const bool live = at < samples, pair = VEC && at + 1 < samples;
    double x[S::ROUNDS];
    /* what term k needs from memory, into x: its window's share, or -- without taps -- this lane's own samples */
    auto fetch = [&](int k) {
        const int T = tap_first[k + 1] - tap_first[k];
        if (T > 0) { blend_filtered_fetch<VEC, HIST>(rows, row_stride, samples, history, hist_stride, channel[k], delay[k], T, tile, x); return; }
        x[0] = x[1] = 0.0;
        if (pair) {
            const v2d p = blend_delayed_load<v2d, HIST>::at(rows, row_stride, history, hist_stride, channel[k], at, delay[k]);
            x[0] = p.x;
            x[1] = p.y;
        } else if (live) {
            x[0] = blend_delayed_load<double, HIST>::at(rows, row_stride, history, hist_stride, channel[k], at, delay[k]);
        }
    };
    auto stage = [&](int k, int buf) {
        if (tap_first[k + 1] == tap_first[k]) return;
#pragma unroll
        for (int r = 0; r < S::ROUNDS; r++) {
            const int m = r * BLEND_T + (int)threadIdx.x;
            if (m < S::WIN) win[buf][m] = x[r];
        }
    };
    fetch(k0);
    stage(k0, 0);
    __syncthreads();
    double s0 = 0.0, s1 = 0.0;
    int cur = 0;
    for (int k = k0; k < k1; k++, cur ^= 1) {
        const int T = tap_first[k + 1] - tap_first[k];
        double f0 = x[0], f1 = x[1];                                        /* a term without taps: its samples, before the next fetch takes x */
        if (k + 1 < k1) fetch(k + 1);                                       /* in flight under this term's taps */
        if (T > 0) {
            const double *__restrict__ h = tap + tap_first[k];
            const double *w = &win[cur][BLEND_F_HALO + l];
            if (VEC) {
                v2d a = *reinterpret_cast<const v2d *>(w);                   /* A_0 */
                f0 = gdg_blend_mul(h[0], a.x);
                f1 = gdg_blend_mul(h[0], a.y);
                for (int t = 1; t < T; t += 2) {
                    const v2d b = *reinterpret_cast<const v2d *>(w - t - 1);  /* A_{t+1}; its first slot is 63 + l - t >= 64 - T >= 0 */
                    f0 = gdg_blend_add(f0, gdg_blend_mul(h[t], b.y));
                    f1 = gdg_blend_add(f1, gdg_blend_mul(h[t], a.x));
                    if (t + 1 < T) {
                        f0 = gdg_blend_add(f0, gdg_blend_mul(h[t + 1], b.x));
                        f1 = gdg_blend_add(f1, gdg_blend_mul(h[t + 1], b.y));
                    }
                    a = b;
                }
            } else {
                f0 = gdg_blend_mul(h[0], w[0]);
                for (int t = 1; t < T; t++) f0 = gdg_blend_add(f0, gdg_blend_mul(h[t], w[-t]));
                f1 = 0.0;
            }
        }
        const double wk = weight[k];
        if (k == k0) {
            s0 = gdg_blend_mul(wk, f0);
            s1 = gdg_blend_mul(wk, f1);
        } else {
            s0 = gdg_blend_add(s0, gdg_blend_mul(wk, f0));
            s1 = gdg_blend_add(s1, gdg_blend_mul(wk, f1));
        }
        if (k + 1 < k1) stage(k + 1, cur ^ 1);
        __syncthreads();                                                     /* every lane is done with win[cur], and win[cur ^ 1] is whole */
    }
    if (pair) {
        const v2d s = { s0, s1 };
        *reinterpret_cast<v2d *>(dst + at) = s;
    } else if (live) {
        dst[at] = s0;
    }
}

template <bool VEC>
__global__ void __launch_bounds__(BLEND_T)
blend_filtered_kernel(const double *rows, size_t row_stride, size_t samples, const int *__restrict__ first, const int *__restrict__ channel,
                      const double *__restrict__ weight, const int *__restrict__ delay, const int *__restrict__ tap_first, const double *__restrict__ tap,
                      const double *history, size_t hist_stride, double *out, size_t out_stride) {
    typedef blend_filtered_shape<VEC> S;
    __shared__ __attribute__((aligned(16))) double win[2][S::WIN];
    const int k0 = first[blockIdx.y], k1 = first[blockIdx.y + 1];
    double *dst = out + (size_t)blockIdx.y * out_stride;
    const size_t tile = (size_t)blockIdx.x * S::TILE;
    if (tile >= (size_t)GDG_BLEND_MAX_DELAY)                                 /* uniform: no slot of this tile's windows lies in front of the launch */
        blend_filtered_tile<VEC, false>(rows, row_stride, samples, channel, weight, delay, tap_first, tap, history, hist_stride, k0, k1, tile, dst, win);
    else
        blend_filtered_tile<VEC, true>(rows, row_stride, samples, channel, weight, delay, tap_first, tap, history, hist_stride, k0, k1, tile, dst, win);
}

/* THE launcher (gdg_internal.h).  d_out: [n_blends][out_stride]; row r at d_rows + r * row_stride.  The table lies in device memory and has
 * been checked by the caller (blend.h: every channel a row of d_rows, 1 to 32 terms a blend, every delay in 0 .. GDG_BLEND_MAX_DELAY, every
 * T at most GDG_BLEND_MAX_TAPS, every d + max(T, 1) - 1 at most GDG_BLEND_MAX_DELAY).  The kernel by what the view holds: taps = filtered,
 * else delays = delayed, else plain -- and the plain kernel reads no history, so none counts there.  d_history: null (+0.0 in front of
 * sample 0) or row r's GDG_BLEND_MAX_DELAY samples in front of sample 0 at d_history + r * hist_stride; read, never written.  d_out overlaps
 * neither the rows nor the history.  A lane takes 16 bytes where every base and stride the kernel reads allows it. */
hipError_t gdg_launch_blend(const gdg_blend_view &v, const double *d_rows, size_t row_stride, size_t samples, const double *d_history, size_t hist_stride, double *d_out,
                            size_t out_stride, hipStream_t s) {
    if (v.n_blends <= 0 || samples == 0) return hipSuccess;
    if (!v.delay) d_history = nullptr;
    if (!d_rows || !d_out || !v.first || !v.channel || !v.weight || (v.tap_first && (!v.delay || !v.tap)) || row_stride < samples || out_stride < samples ||
        v.n_blends > 65535 || ((uintptr_t)d_rows & 7) || ((uintptr_t)d_out & 7) || ((uintptr_t)v.weight & 7) || ((uintptr_t)v.tap & 7) || ((uintptr_t)v.first & 3) ||
        ((uintptr_t)v.channel & 3) || ((uintptr_t)v.delay & 3) || ((uintptr_t)v.tap_first & 3) ||
        (d_history && (((uintptr_t)d_history & 7) || hist_stride < (size_t)GDG_BLEND_MAX_DELAY)))
        return hipErrorInvalidValue;
    const bool vec = !((uintptr_t)d_rows & 15) && !(row_stride & 1) && !((uintptr_t)d_out & 15) && !(out_stride & 1) &&
                     (!d_history || (!((uintptr_t)d_history & 15) && !(hist_stride & 1)));
    const size_t lanes = vec ? (samples + 1) / 2 : samples, tiles = (lanes + BLEND_T - 1) / BLEND_T;
    if (tiles > 0x7fffffffu) return hipErrorInvalidValue;
    const dim3 grid((unsigned)tiles, (unsigned)v.n_blends);
    if (v.tap_first) {
        if (vec) blend_filtered_kernel<true><<<grid, BLEND_T, 0, s>>>(d_rows, row_stride, samples, v.first, v.channel, v.weight, v.delay, v.tap_first, v.tap, d_history, hist_stride, d_out, out_stride);
        else blend_filtered_kernel<false><<<grid, BLEND_T, 0, s>>>(d_rows, row_stride, samples, v.first, v.channel, v.weight, v.delay, v.tap_first, v.tap, d_history, hist_stride, d_out, out_stride);
    } else if (v.delay) {
        if (vec) blend_delayed_kernel<true><<<grid, BLEND_T, 0, s>>>(d_rows, row_stride, samples, v.first, v.channel, v.weight, v.delay, d_history, hist_stride, d_out, out_stride);
        else blend_delayed_kernel<false><<<grid, BLEND_T, 0, s>>>(d_rows, row_stride, samples, v.first, v.channel, v.weight, v.delay, d_history, hist_stride, d_out, out_stride);
    } else {
        if (vec) blend_rows_kernel<true><<<grid, BLEND_T, 0, s>>>(d_rows, row_stride, samples, v.first, v.channel, v.weight, d_out, out_stride);
        else blend_rows_kernel<false><<<grid, BLEND_T, 0, s>>>(d_rows, row_stride, samples, v.first, v.channel, v.weight, d_out, out_stride);
    }
    return hipGetLastError();
}
