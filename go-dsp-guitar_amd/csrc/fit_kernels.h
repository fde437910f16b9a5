/*
 * fit_kernels.h -- the blend fit's record (include/gdg.h, FIT): per fit and block the Gram matrix of up to 8 rows and
 * their inner products with a target row -- what a least-squares fit of blend weights needs, taken from the float64 rows where they lie.
 * No reference counterpart.  Included by io.hip behind block_stats_kernel, whose order of sums it restates for every entry, and compiled
 * like it without contraction.
 *
 * One workgroup of 256 threads per (block, fit): blockIdx.x = block, blockIdx.y = fit.  The fit's table entry -- target | terms | port[8] --
 * is read at addresses that depend on blockIdx.y alone (scalar loads), and the term count K it holds is the same for the whole workgroup.
 * The kernel is instantiated per K, unrolled for exactly K terms and with the registers of K terms -- a fit of two terms runs 6 sums in a
 * kernel of 6 sums, not 45 --: the launcher launches the instantiation of every K the list holds over the whole grid, and a workgroup whose
 * fit has another K leaves at once (a list's fits usually share one K: one launch).
 *   thread t walks the sample pairs p = t, t + 256 ... (2 p < L), the samples 2 p and 2 p + 1 of each one after the other, into ONE running
 *   sum per entry; a sample index at which any of the K + 1 rows is NaN or +-inf adds to no sum and counts as skipped;
 *   the 64 lanes of a wave meet in the fixed tree lane i <- lane i + 32, + 16 .. + 1; the four wave results through LDS, added 0, 1, 2, 3.
 * Every product is __dmul_rn and every add __dadd_rn; no atomics.  With nothing skipped the diagonal entry of term k is therefore bit for
 * bit block_stats_kernel's sum_sq of that row and block, and xx is the same under an exchange of two terms (a product commutes).
 * VEC reads a pair of every row with one 16-byte load where the launcher has seen that every block of every row starts 16-byte aligned
 * and `block` is even; the values and their order are the scalar path's.  A pair's second sample is read only when it lies inside the
 * block: nothing outside [row, row + samples).  Plain loads: the encoder reads the same rows next.
 */
#define FIT_T 256
#define FIT_SUMS 45                            /* tt | tx[8] | xx[36]: the doubles of a gdg_block_fit */
#define FIT_RECORD_DOUBLES 46                  /* ... and (skipped, terms) as the 46th */
static_assert(FIT_SUMS == 1 + GDG_FIT_MAX_TERMS + GDG_FIT_MAX_TERMS * (GDG_FIT_MAX_TERMS + 1) / 2 && FIT_RECORD_DOUBLES * 8 == sizeof(gdg_block_fit),
              "a gdg_block_fit is 45 sums and two counts");

/* one sample index of the K + 1 rows (v[0] = the target, v[1 + k] = term k) into the thread's sums: acc = tt | tx[K] | xx[K (K + 1) / 2] */
template <int K>
__device__ __forceinline__ void fit_take(double *acc, unsigned &skipped, const double *v) {
    bool finite = true;
#pragma unroll
    for (int r = 0; r <= K; r++) finite = finite && fabs(v[r]) <= 1.7976931348623157e308;      /* false for NaN and for +-inf */
    if (!finite) { skipped++; return; }
    acc[0] = __dadd_rn(acc[0], __dmul_rn(v[0], v[0]));
#pragma unroll
    for (int k = 0; k < K; k++) acc[1 + k] = __dadd_rn(acc[1 + k], __dmul_rn(v[0], v[1 + k]));
#pragma unroll
    for (int j = 0; j < K; j++)
#pragma unroll
        for (int k = 0; k <= j; k++) acc[1 + K + j * (j + 1) / 2 + k] = __dadd_rn(acc[1 + K + j * (j + 1) / 2 + k], __dmul_rn(v[1 + j], v[1 + k]));
}

template <bool VEC, int K>
__device__ __forceinline__ void block_fit_body(const double *__restrict__ rows, size_t row_stride, size_t first, unsigned L, const int *__restrict__ fit,
                                               double *__restrict__ rec, double (*s_sum)[FIT_SUMS], unsigned *s_skip) {
    constexpr int E = 1 + K + K * (K + 1) / 2;
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    const double *x[K + 1];
    x[0] = rows + (size_t)(unsigned)fit[0] * row_stride + first;
#pragma unroll
    for (int k = 0; k < K; k++) x[1 + k] = rows + (size_t)(unsigned)fit[2 + k] * row_stride + first;
    double acc[E];
#pragma unroll
    for (int e = 0; e < E; e++) acc[e] = 0.0;
    unsigned skipped = 0u;
    /* PAIRS pairs of every row per round, their loads in flight together; the sums follow in the pairs' order */
    constexpr int PAIRS = K <= 2 ? 4 : (K <= 4 ? 2 : 1);
    for (unsigned p0 = tid; 2u * p0 < L; p0 += (unsigned)PAIRS * FIT_T) {
        double v[PAIRS][2][K + 1];
#pragma unroll
        for (int q = 0; q < PAIRS; q++) {
            const unsigned i = 2u * (p0 + (unsigned)q * FIT_T);
#pragma unroll
            for (int r = 0; r <= K; r++) {
                v[q][0][r] = v[q][1][r] = 0.0;
                if (VEC && i + 1u < L) {
                    const v2d pair = *reinterpret_cast<const v2d *>(x[r] + i);
                    v[q][0][r] = pair.x;
                    v[q][1][r] = pair.y;
                } else {
                    if (i < L) v[q][0][r] = x[r][i];
                    if (i + 1u < L) v[q][1][r] = x[r][i + 1u];
                }
            }
        }
#pragma unroll
        for (int q = 0; q < PAIRS; q++) {
            const unsigned i = 2u * (p0 + (unsigned)q * FIT_T);
            if (i < L) fit_take<K>(acc, skipped, v[q][0]);
            if (i + 1u < L) fit_take<K>(acc, skipped, v[q][1]);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int e = 0; e < E; e++) acc[e] = __dadd_rn(acc[e], __shfl_down(acc[e], o));
        skipped += __shfl_down(skipped, o);
    }
    if (lane == 0) {
        const unsigned w = tid >> 6;
#pragma unroll
        for (int e = 0; e < E; e++) s_sum[w][e] = acc[e];
        s_skip[w] = skipped;
    }
    __syncthreads();
    /* the record: thread e writes its e-th double -- the waves' sums added 0, 1, 2, 3; +0.0 for a term the fit does not have -- and thread
     * 45 the two counts */
    if (tid < FIT_SUMS) {
        const int e = (int)tid;
        int at = -1;                                                         /* the entry's place among the E sums a wave left */
        if (e == 0) at = 0;
        else if (e <= GDG_FIT_MAX_TERMS) { if (e - 1 < K) at = e; }
        else if (e - 1 - GDG_FIT_MAX_TERMS < K * (K + 1) / 2) at = 1 + K + (e - 1 - GDG_FIT_MAX_TERMS);
        double s = 0.0;
        if (at >= 0) {
            s = s_sum[0][at];
#pragma unroll
            for (int w = 1; w < FIT_T / 64; w++) s = __dadd_rn(s, s_sum[w][at]);
        }
        rec[e] = s;
    } else if (tid == FIT_SUMS) {
        unsigned n = s_skip[0];
#pragma unroll
        for (int w = 1; w < FIT_T / 64; w++) n += s_skip[w];
        rec[FIT_SUMS] = __longlong_as_double((long long)(((unsigned long long)(unsigned)K << 32) | (unsigned long long)n));      /* skipped, then terms: little-endian */
    }
}

template <bool VEC, int K>
__global__ void __launch_bounds__(FIT_T)
block_fit_kernel(const double *__restrict__ rows, size_t row_stride, size_t samples, unsigned block, unsigned blocks_per_row, const int *__restrict__ table,
                 double *__restrict__ records) {
    __shared__ double s_sum[FIT_T / 64][FIT_SUMS];
    __shared__ unsigned s_skip[FIT_T / 64];
    const int *fit = table + (size_t)blockIdx.y * GDG_FIT_TABLE_INTS;
    if (fit[1] != K) return;                                                 /* another instantiation's fit: one value for the whole workgroup */
    const size_t first = (size_t)blockIdx.x * block;
    const unsigned L = (unsigned)(samples - first < (size_t)block ? samples - first : (size_t)block);
    double *rec = records + ((size_t)blockIdx.y * blocks_per_row + blockIdx.x) * FIT_RECORD_DOUBLES;
    block_fit_body<VEC, K>(rows, row_stride, first, L, fit, rec, s_sum, s_skip);
}

template <int K>
static void launch_block_fit(bool vec, dim3 grid, const double *d_rows, size_t row_stride, size_t samples, unsigned block, unsigned blocks, const int *d_table,
                             double *out, hipStream_t s) {
    if (vec) block_fit_kernel<true, K><<<grid, FIT_T, 0, s>>>(d_rows, row_stride, samples, block, blocks, d_table, out);
    else block_fit_kernel<false, K><<<grid, FIT_T, 0, s>>>(d_rows, row_stride, samples, block, blocks, d_table, out);
}

/* d_records: [n_fits][ceil(samples / block)] records of 368 bytes.  h_table is the host's copy of the n_fits entries at d_table -- target |
 * terms | port[8] each --, checked here against n_rows before anything is launched: the kernel reads rows by what the table says */
hipError_t gdg_launch_block_fit(const double *d_rows, size_t row_stride, unsigned n_rows, size_t samples, unsigned block, const int *h_table, const int *d_table,
                                unsigned n_fits, void *d_records, hipStream_t s) {
    if (n_fits == 0 || samples == 0) return hipSuccess;
    if (block == 0 || n_fits > GDG_FIT_MAX_FITS || !h_table || !d_table) return hipErrorInvalidValue;
    unsigned held = 0u;                                                      /* bit K: some fit of the list has K terms */
    for (unsigned f = 0; f < n_fits; f++) {
        const int *e = h_table + (size_t)f * GDG_FIT_TABLE_INTS;
        if (e[0] < 0 || (unsigned)e[0] >= n_rows || e[1] < 1 || e[1] > GDG_FIT_MAX_TERMS) return hipErrorInvalidValue;
        for (int k = 0; k < e[1]; k++) if (e[2 + k] < 0 || (unsigned)e[2 + k] >= n_rows) return hipErrorInvalidValue;
        held |= 1u << e[1];
    }
    const size_t blocks = (samples + block - 1) / block;
    if (row_stride < samples || blocks > 0x7fffffffu || ((uintptr_t)d_rows & 7) || ((uintptr_t)d_records & 7) || ((uintptr_t)d_table & 3)) return hipErrorInvalidValue;
    const bool vec = !((uintptr_t)d_rows & 15) && !(row_stride & 1) && !(block & 1);
    const dim3 grid((unsigned)blocks, n_fits);
    double *out = static_cast<double *>(d_records);
    if (held & (1u << 1)) launch_block_fit<1>(vec, grid, d_rows, row_stride, samples, block, (unsigned)blocks, d_table, out, s);
    if (held & (1u << 2)) launch_block_fit<2>(vec, grid, d_rows, row_stride, samples, block, (unsigned)blocks, d_table, out, s);
    if (held & (1u << 3)) launch_block_fit<3>(vec, grid, d_rows, row_stride, samples, block, (unsigned)blocks, d_table, out, s);
    if (held & (1u << 4)) launch_block_fit<4>(vec, grid, d_rows, row_stride, samples, block, (unsigned)blocks, d_table, out, s);
    if (held & (1u << 5)) launch_block_fit<5>(vec, grid, d_rows, row_stride, samples, block, (unsigned)blocks, d_table, out, s);
    if (held & (1u << 6)) launch_block_fit<6>(vec, grid, d_rows, row_stride, samples, block, (unsigned)blocks, d_table, out, s);
    if (held & (1u << 7)) launch_block_fit<7>(vec, grid, d_rows, row_stride, samples, block, (unsigned)blocks, d_table, out, s);
    if (held & (1u << 8)) launch_block_fit<8>(vec, grid, d_rows, row_stride, samples, block, (unsigned)blocks, d_table, out, s);
    return hipGetLastError();
}
