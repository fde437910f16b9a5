/*
 * delivered_kernels.h -- the records of the delivered rows (include/gdg.h, DELIVERED RECORDS): peak, sum of squares and a
 * true peak that is seamless across blocks, of rows cut into blocks of any length from 1 to 16384 samples.  Included by io.hip behind the
 * delivery kernels and compiled like them without contraction.
 *
 * block_delivered_kernel: one workgroup of 256 threads per (block, row): blockIdx.x = block k, blockIdx.y = row.  Block k of a row is its
 * samples span[k] <= i < span[k + 1] (a device array, the same for every row); o = span[k], L = its length.
 *   - the block is walked in tiles of DELIVERED_TILE = 2048 samples staged in LDS behind a lead-in of the 23 samples in front of the tile
 *     (24 slots, the first idle, so that a pair of samples stays one 16-byte slot): 2072 doubles = 16 576 bytes, whatever L is.
 *   - a tile is four rounds of 256 pairs: thread t takes the pairs t, t + 256, t + 512, t + 768 of the tile, their loads in flight together,
 *     then the next tile's: over the block the pairs t, t + 256, t + 512 .. in ascending order into ONE running sum and one running
 *     (peak, index) -- block_stats_kernel's order at L, so sum_sq has its bits.  The load rule is that kernel's: a pair per 16-byte load where
 *     the launcher has seen that the rows allow it (`vec`) and the block begins at an even sample, two 8-byte loads otherwise -- the same
 *     values.  A sample is read only when it lies inside the block, the lead-in only inside the row: nothing outside [row, row + samples).
 *   - the lead-in comes from the row where it has the samples, from the history's 23 doubles in front of the launch (null: +0.0) otherwise.
 *     Non-finite samples are zeroed on the way in, the lead-in's too.
 *   - behind a barrier thread t walks the tile's samples c = t, t + 256 ..: the interval n = c - 12 is the one whose last sample is c, and
 *     v_p = sum_k x[c - 23 + k] h_p[k] from 0.0 in ascending k, every product and add rounded on its own (tp_mac).  The 72 taps are a kernel
 *     argument: uniform, fetched by scalar loads.  Consecutive lanes read consecutive 8-byte words of LDS: every bank once per half wave.
 *   - the 64 lanes meet in the fixed tree lane i <- lane i + 32, + 16 .. + 1, the four waves through LDS in wave order; sums as (mine +
 *     theirs); "better" is lexicographic at every level.  No atomics; the record leaves as vector stores from thread 0.
 *
 * delivered_history_save_kernel: the last 23 samples of (history ++ the launch's samples) into the history, read -- barrier -- write, so a
 * launch of fewer than 23 samples moves the old ones up in place.
 *
 * Both have C linkage: two tests take their census of io.hip's delivery kernels by their C++-mangled names.
 */
#define DELIVERED_T 256
#define DELIVERED_TILE 2048
#define DELIVERED_LEAD 24
#define GDG_DELIVERED_HISTORY 23
#define GDG_DELIVERED_MAX_BLOCK 16384

static_assert(GDG_DELIVERED_HISTORY == GDG_TRUE_PEAK_TAPS - 1 && DELIVERED_LEAD == GDG_TRUE_PEAK_TAPS, "the lead-in is what the interval that ends with a tile's first sample reads in front of it");
static_assert(DELIVERED_TILE % (2 * DELIVERED_T) == 0, "a tile holds a whole number of 256-pair rounds");

struct DeliveredAcc { double peak, ssq, m; unsigned idx, clipped, overs; int pos; };

__device__ __forceinline__ void delivered_sample(DeliveredAcc &a, double x, unsigned i) {
    const double m = fabs(x);
    if (m > a.peak) { a.peak = m; a.idx = i; }
    a.ssq = __dadd_rn(a.ssq, __dmul_rn(x, x));
    a.clipped += m > 1.0 ? 1u : 0u;
}
__device__ __forceinline__ void delivered_point(DeliveredAcc &a, double m, int pos) {
    if (m > a.m || (m == a.m && pos < a.pos)) { a.m = m; a.pos = pos; }
}
__device__ __forceinline__ void delivered_join(DeliveredAcc &a, double peak, unsigned idx, double ssq, unsigned clipped, double m, int pos, unsigned overs) {
    if (peak > a.peak || (peak == a.peak && idx < a.idx)) { a.peak = peak; a.idx = idx; }
    a.ssq = __dadd_rn(a.ssq, ssq);
    a.clipped += clipped;
    delivered_point(a, m, pos);
    a.overs += overs;
}

extern "C" __global__ void __launch_bounds__(DELIVERED_T)
block_delivered_kernel(const double *__restrict__ rows, size_t row_stride, size_t samples, const unsigned long long *__restrict__ span, unsigned row0, unsigned blocks_per_row,
                       const double *__restrict__ history, const gdg_true_peak_table taps, gdg_block_delivered *__restrict__ records, int vec) {
    constexpr int NT = GDG_TRUE_PEAK_TAPS, NP = GDG_TRUE_PEAK_PHASES, H = GDG_TRUE_PEAK_H, NW = DELIVERED_T / 64, ROUNDS = DELIVERED_TILE / (2 * DELIVERED_T);
    __shared__ double s_x[DELIVERED_LEAD + DELIVERED_TILE];
    __shared__ double s_peak[NW], s_ssq[NW], s_m[NW];
    __shared__ unsigned s_idx[NW], s_cnt[NW][2];
    __shared__ int s_pos[NW];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const unsigned row = row0 + blockIdx.y;
    const double *x_row = rows + (size_t)row * row_stride;
    const double *hist = history ? history + (size_t)row * GDG_DELIVERED_HISTORY : nullptr;
    /* the launcher has held the spans against the row; the kernel does so again, so that whatever they hold nothing outside the row is read */
    unsigned long long o = span[blockIdx.x], e = span[blockIdx.x + 1];
    if (e > samples) e = samples;
    if (o > e) o = e;
    const int L = (int)(e - o < (unsigned long long)GDG_DELIVERED_MAX_BLOCK ? e - o : (unsigned long long)GDG_DELIVERED_MAX_BLOCK);
    const double *x = x_row + o;
    const bool pairs = vec && !(o & 1ull);

    DeliveredAcc a = { 0.0, 0.0, 0.0, 0u, 0u, 0u, 0 };
    for (int t0 = 0; t0 < L; t0 += DELIVERED_TILE) {
        const int TL = L - t0 < DELIVERED_TILE ? L - t0 : DELIVERED_TILE;
        /* the 23 samples in front of the tile: the row's where it has them, the history's in front of the launch */
        if (tid < GDG_DELIVERED_HISTORY) {
            const long long s = (long long)o + t0 - GDG_DELIVERED_HISTORY + tid;
            double v = 0.0;
            if (s >= 0) v = x_row[s];
            else if (hist) v = hist[GDG_DELIVERED_HISTORY + s];
            s_x[1 + tid] = tp_finite(v);
        }
        /* the tile, pair by pair: four pairs per thread, their loads in flight together; the sums follow in the pairs' order */
        double v[ROUNDS][2];
#pragma unroll
        for (int k = 0; k < ROUNDS; k++) {
            const int i = 2 * (k * DELIVERED_T + tid);
            v[k][0] = v[k][1] = 0.0;
            if (pairs && i + 1 < TL) {
                const v2d q = *reinterpret_cast<const v2d *>(x + t0 + i);
                v[k][0] = q.x;
                v[k][1] = q.y;
            } else {
                if (i < TL) v[k][0] = x[t0 + i];
                if (i + 1 < TL) v[k][1] = x[t0 + i + 1];
            }
        }
#pragma unroll
        for (int k = 0; k < ROUNDS; k++) {
            const int i = 2 * (k * DELIVERED_T + tid);
            if (i < TL) {
                const double v0 = tp_finite(v[k][0]);
                s_x[DELIVERED_LEAD + i] = v0;
                delivered_sample(a, v0, (unsigned)(t0 + i));
            }
            if (i + 1 < TL) {
                const double v1 = tp_finite(v[k][1]);
                s_x[DELIVERED_LEAD + i + 1] = v1;
                delivered_sample(a, v1, (unsigned)(t0 + i + 1));
            }
        }
        __syncthreads();
        /* the intervals that complete in the tile: the one that ends with sample c reads the slots 1 + c .. 24 + c */
        for (int c = tid; c < TL; c += DELIVERED_T) {
            double xs[NT];
#pragma unroll
            for (int k = 0; k < NT; k++) xs[k] = s_x[1 + c + k];
            const int n = t0 + c - H;
#pragma unroll
            for (int p = 0; p < NP; p++) {
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < NT; k++) acc = tp_mac(acc, xs[k], taps.h[p][k]);
                const double m = fabs(acc);
                delivered_point(a, m, 4 * n + p + 1);
                a.overs += m > 1.0 ? 1u : 0u;
            }
        }
        __syncthreads();                                                    /* the next tile overwrites what was just read */
    }
    /* the thread's own samples join its points: its first largest sample at position 4 i */
    delivered_point(a, a.peak, 4 * (int)a.idx);

#pragma unroll
    for (int s = 32; s > 0; s >>= 1)
        delivered_join(a, __shfl_down(a.peak, s), __shfl_down(a.idx, s), __shfl_down(a.ssq, s), __shfl_down(a.clipped, s), __shfl_down(a.m, s), __shfl_down(a.pos, s),
                       __shfl_down(a.overs, s));
    if (lane == 0) {
        const int w = tid >> 6;
        s_peak[w] = a.peak; s_ssq[w] = a.ssq; s_m[w] = a.m; s_idx[w] = a.idx; s_pos[w] = a.pos;
        s_cnt[w][0] = a.clipped; s_cnt[w][1] = a.overs;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < NW; w++) delivered_join(a, s_peak[w], s_idx[w], s_ssq[w], s_cnt[w][0], s_m[w], s_pos[w], s_cnt[w][1]);
        gdg_block_delivered *r = records + (size_t)row * blocks_per_row + blockIdx.x;
        r->true_peak = a.m;
        r->peak = a.peak;
        r->sum_sq = a.ssq;
        r->position = a.m > 0.0 ? a.pos : 0;
        r->peak_index = a.idx;
        r->overs = a.overs;
        r->clipped = a.clipped;
    }
}

extern "C" __global__ void __launch_bounds__(64)
delivered_history_save_kernel(const double *rows, size_t row_stride, size_t samples, double *history) {
    const int j = (int)threadIdx.x;
    double *hist = history + (size_t)blockIdx.x * GDG_DELIVERED_HISTORY;
    double v = 0.0;
    if (j < GDG_DELIVERED_HISTORY) {
        const long long s = (long long)samples - GDG_DELIVERED_HISTORY + j;     /* the launch's sample that becomes entry j */
        v = s >= 0 ? rows[(size_t)blockIdx.x * row_stride + (size_t)s] : hist[GDG_DELIVERED_HISTORY + s];
    }
    __syncthreads();
    if (j < GDG_DELIVERED_HISTORY) hist[j] = v;
}

/* n_rows rows of `samples` float64 (row r at d_rows + r * row_stride, 8-byte aligned), cut by d_span[0 .. n_blocks] -- ascending, d_span[0] = 0,
 * d_span[n_blocks] = samples, every length 1 to 16384: the caller has held the host's copy against that -- into n_blocks blocks a row;
 * d_history: null (+0.0 in front of the launch) or [n_rows][23], read only.  d_out: [n_rows][n_blocks] records of 40 bytes. */
hipError_t gdg_launch_block_delivered(const double *d_rows, size_t row_stride, unsigned n_rows, size_t samples, const unsigned long long *d_span, unsigned n_blocks,
                                      const double *d_history, const gdg_true_peak_table &taps, void *d_out, hipStream_t s) {
    gdg_block_delivered *d_records = static_cast<gdg_block_delivered *>(d_out);
    if (n_rows == 0 || n_blocks == 0) return hipSuccess;
    if (!d_rows || !d_span || !d_records || samples == 0 || row_stride < samples || n_blocks > 0x7fffffffu || ((uintptr_t)d_rows & 7) || ((uintptr_t)d_records & 7) ||
        ((uintptr_t)d_history & 7) || ((uintptr_t)d_span & 7))
        return hipErrorInvalidValue;
    const bool vec = !((uintptr_t)d_rows & 15) && !(row_stride & 1);
    for (unsigned r0 = 0; r0 < n_rows; r0 += 65535u) {                      /* gridDim.y holds 65535 rows */
        const dim3 grid(n_blocks, n_rows - r0 < 65535u ? n_rows - r0 : 65535u);
        block_delivered_kernel<<<grid, DELIVERED_T, 0, s>>>(d_rows, row_stride, samples, d_span, r0, n_blocks, d_history, taps, d_records, vec ? 1 : 0);
    }
    return hipGetLastError();
}

/* behind the launch above and before anything writes the rows again: d_history[n_rows][23] takes the last 23 samples of (history ++ rows) */
hipError_t gdg_launch_delivered_history_save(const double *d_rows, size_t row_stride, size_t samples, unsigned n_rows, double *d_history, hipStream_t s) {
    if (n_rows == 0 || samples == 0) return hipSuccess;
    if (!d_rows || !d_history || row_stride < samples || ((uintptr_t)d_rows & 7) || ((uintptr_t)d_history & 7)) return hipErrorInvalidValue;
    delivered_history_save_kernel<<<n_rows, 64, 0, s>>>(d_rows, row_stride, samples, d_history);
    return hipGetLastError();
}
