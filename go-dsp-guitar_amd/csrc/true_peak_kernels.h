/*
 * true_peak_kernels.h -- the true-peak record of the render report (include/gdg.h, gdg_block_true_peak_rows): the largest
 * magnitude of a block's samples and of the three points a 24-tap windowed-sinc interpolator puts between two of them.  No reference
 * counterpart, and no transform: included by io.hip, next to block_stats_kernel, and compiled like it without contraction.
 *
 * One workgroup of 256 threads per (block, row): blockIdx.x = block, blockIdx.y = row.  The block is staged in LDS (64 KiB, unpadded:
 * consecutive lanes read consecutive 8-byte words, so a wave's read touches every bank once per half), non-finite samples zeroed on the way
 * in, with block_stats_kernel's load rule: a pair per 16-byte load where the launcher has seen that every block starts 16-byte aligned, two
 * 8-byte loads otherwise -- the same values.  A sample is read only when it lies inside the block: nothing outside [row, row + samples).
 * Thread t then walks the samples t, t + 256 .. (position 4 i) and the intervals n = H - 1 + t, + 256 .. <= L - H - 1 (positions
 * 4 n + 1, 2, 3): v = sum_j x[n + j] h[j] from 0.0 in ascending j, every product and every add rounded on its own (tp_mac).  The 72 taps
 * are a kernel argument: uniform, fetched by scalar loads.  Running (|v|, position) and the count of |v| > 1 are per thread; the 64 lanes
 * meet in the fixed tree lane i <- lane i + 32, + 16 .. + 1, the four waves through LDS in wave order; "better" is lexicographic at every
 * level -- greater |v|, then the lower position -- so the record is a function of the block's samples alone.  No atomics; the record
 * leaves as vector stores from thread 0.
 */
#define TRUE_PEAK_T 256

struct TruePeakAcc { double m; unsigned pos, overs; };

__device__ __forceinline__ void tp_take(TruePeakAcc &a, double m, unsigned pos) {
    if (m > a.m || (m == a.m && pos < a.pos)) { a.m = m; a.pos = pos; }
}

/* acc + x h, the product and the add each rounded on its own: written as an add under the file's contraction-off, which cannot take the
 * product in, rather than as two intrinsics side by side */
__device__ __forceinline__ double tp_mac(double acc, double x, double h) { return acc + __dmul_rn(x, h); }

__device__ __forceinline__ double tp_finite(double x) { return fabs(x) <= 1.7976931348623157e308 ? x : 0.0; }     /* NaN, +-inf: 0 */

template <bool VEC>
__global__ void __launch_bounds__(TRUE_PEAK_T)
block_true_peak_kernel(const double *__restrict__ rows, size_t row_stride, size_t samples, unsigned row0, unsigned blocks_per_row,
                       const gdg_true_peak_table taps, gdg_block_true_peak *__restrict__ records) {
    constexpr int H = GDG_TRUE_PEAK_H, NT = GDG_TRUE_PEAK_TAPS, NP = GDG_TRUE_PEAK_PHASES, NW = TRUE_PEAK_T / 64;
    __shared__ double s_x[GDG_TRUE_PEAK_BLOCK];
    __shared__ double s_m[NW];
    __shared__ unsigned s_pos[NW], s_overs[NW];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const unsigned row = row0 + blockIdx.y;
    const size_t first = (size_t)blockIdx.x * GDG_TRUE_PEAK_BLOCK;
    const int L = (int)(samples - first < (size_t)GDG_TRUE_PEAK_BLOCK ? samples - first : (size_t)GDG_TRUE_PEAK_BLOCK);
    const double *x = rows + (size_t)row * row_stride + first;

    TruePeakAcc a = { 0.0, 0u, 0u };
    /* the block into LDS, pair by pair, and the samples' own magnitudes on the way */
#pragma unroll 4
    for (int i = 2 * tid; i < L; i += 2 * TRUE_PEAK_T) {
        double v0 = 0.0, v1 = 0.0;
        if (VEC && i + 1 < L) {
            const v2d q = *reinterpret_cast<const v2d *>(x + i);
            v0 = q.x;
            v1 = q.y;
        } else {
            v0 = x[i];
            if (i + 1 < L) v1 = x[i + 1];
        }
        v0 = tp_finite(v0);
        v1 = tp_finite(v1);
        s_x[i] = v0;
        tp_take(a, fabs(v0), 4u * (unsigned)i);
        if (i + 1 < L) {
            s_x[i + 1] = v1;
            tp_take(a, fabs(v1), 4u * (unsigned)(i + 1));
        }
    }
    __syncthreads();

    /* the intervals whose 24 samples n - H + 1 .. n + H lie inside the block */
    for (int n = H - 1 + tid; n + H < L; n += TRUE_PEAK_T) {
        double xs[NT];
#pragma unroll
        for (int k = 0; k < NT; k++) xs[k] = s_x[n - (H - 1) + k];
#pragma unroll
        for (int p = 0; p < NP; p++) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < NT; k++) acc = tp_mac(acc, xs[k], taps.h[p][k]);
            const double m = fabs(acc);
            tp_take(a, m, 4u * (unsigned)n + (unsigned)(p + 1));
            a.overs += m > 1.0 ? 1u : 0u;
        }
    }

#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double m = __shfl_down(a.m, o);
        const unsigned pos = __shfl_down(a.pos, o);
        a.overs += __shfl_down(a.overs, o);
        tp_take(a, m, pos);
    }
    if (lane == 0) { s_m[tid >> 6] = a.m; s_pos[tid >> 6] = a.pos; s_overs[tid >> 6] = a.overs; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < NW; w++) { tp_take(a, s_m[w], s_pos[w]); a.overs += s_overs[w]; }
        gdg_block_true_peak *r = records + (size_t)row * blocks_per_row + blockIdx.x;
        r->true_peak = a.m;
        r->position = a.m > 0.0 ? a.pos : 0u;
        r->overs = a.overs;
    }
}

/* d_out: [n_rows][ceil(samples / 8192)] records of 16 bytes; row r at d_rows + r * row_stride */
hipError_t gdg_launch_block_true_peak(const double *d_rows, size_t row_stride, unsigned n_rows, size_t samples, const gdg_true_peak_table &taps, void *d_out,
                                      hipStream_t s) {
    gdg_block_true_peak *d_records = static_cast<gdg_block_true_peak *>(d_out);
    if (n_rows == 0 || samples == 0) return hipSuccess;
    const size_t blocks = (samples + GDG_TRUE_PEAK_BLOCK - 1) / GDG_TRUE_PEAK_BLOCK;
    if (row_stride < samples || blocks > 0x7fffffffu || ((uintptr_t)d_rows & 7) || ((uintptr_t)d_records & 7)) return hipErrorInvalidValue;
    const bool vec = !((uintptr_t)d_rows & 15) && !(row_stride & 1);
    for (unsigned r0 = 0; r0 < n_rows; r0 += 65535u) {                      /* gridDim.y holds 65535 rows */
        const dim3 grid((unsigned)blocks, n_rows - r0 < 65535u ? n_rows - r0 : 65535u);
        if (vec) block_true_peak_kernel<true><<<grid, TRUE_PEAK_T, 0, s>>>(d_rows, row_stride, samples, r0, (unsigned)blocks, taps, d_records);
        else block_true_peak_kernel<false><<<grid, TRUE_PEAK_T, 0, s>>>(d_rows, row_stride, samples, r0, (unsigned)blocks, taps, d_records);
    }
    return hipGetLastError();
}
