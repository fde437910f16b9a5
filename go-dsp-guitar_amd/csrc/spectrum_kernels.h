/*
 * spectrum_kernels.h -- the band spectrum of the render report (include/gdg.h, gdg_block_spectrum_rows).  No reference
 * counterpart.  Included at the end of fir.hip, like tuner_kernels.h, because it reuses the register/LDS Stockham passes defined there
 * -- but in front of the tuner's pragma: this code is compiled without contraction, like the transforms.
 *
 * One workgroup of 256 threads per (block, row): blockIdx.x = block, blockIdx.y = row.  The block's 8192 samples times the periodic
 * Hann window are the packed input of ONE 4096-point complex transform (FftCfg<12>: 16 points per thread, 68.25 KiB of LDS, two
 * workgroups per CU), un-packed to the real sequence's bins k = 0 .. 4096 as fir_fwd_kernel and the tuner do.  c_k |X[k]|^2 replaces
 * Z in LDS (a thread writes only the two entries it alone has read), and wave v sums the bands v, v + 4, v + 8 ..:
 *   lane l adds the bins k_lo + l, k_lo + l + 64 .. < k_hi in ascending order into one running sum; the 64 lanes meet in the fixed tree
 *   lane i <- lane i + 32, + 16 .. + 1; lane 0 divides by L^2 3/8 = 25165824 and stores.
 * A band lives on one wave, so no partial sum crosses waves.  Every square and every add is __dmul_rn / __dadd_rn; the order is a function
 * of (k_lo, k_hi) alone -- not of the row, the grid, the block's place, the window, the slice or the shard.  VEC reads a pair of samples
 * with one 16-byte load where the launcher has seen that every block starts 16-byte aligned; the values are the scalar path's.  A sample
 * is read only when it lies inside the block: nothing outside [row, row + samples); a short last block is zero-padded in registers.
 */
#define SPECTRUM_LOGN 12
#define SPECTRUM_SCALE 25165824.0                 /* L^2 * 3/8, L = 8192 */

__device__ __forceinline__ double spectrum_finite(double x) { return fabs(x) <= 1.7976931348623157e308 ? x : 0.0; }     /* NaN, +-inf: 0 */
__device__ __forceinline__ double spectrum_sq(cplx z) { return __dadd_rn(__dmul_rn(z.x, z.x), __dmul_rn(z.y, z.y)); }

template <bool VEC>
__global__ void __launch_bounds__(FftCfg<SPECTRUM_LOGN>::T)
block_spectrum_kernel(const double *__restrict__ rows, size_t row_stride, size_t samples, unsigned row0, unsigned blocks_per_row,
                      const double *__restrict__ win, const cplx *__restrict__ tw, const cplx *__restrict__ tw2, gdg_spectrum_bands bands,
                      double *__restrict__ out) {
    constexpr int LOGN = SPECTRUM_LOGN, N = FftCfg<LOGN>::N, T = FftCfg<LOGN>::T, ITER = (N / 2) / T;
    constexpr int LR0 = sched_lr(LOGN, 0), R0 = 1 << LR0, B0 = 16 / R0;
    static_assert(2 * N == GDG_SPECTRUM_BLOCK && GDG_PAD(N) < FftCfg<LOGN>::LDS, "8192 reals as 4096 packed points; bin N has a place in LDS");
    __shared__ double s_all[2 * FftCfg<LOGN>::LDS];
    double *sre = s_all, *sim = s_all + FftCfg<LOGN>::LDS;
    const int tid = threadIdx.x;
    const unsigned row = row0 + blockIdx.y;
    const size_t first = (size_t)blockIdx.x * GDG_SPECTRUM_BLOCK;
    const int L = (int)(samples - first < (size_t)GDG_SPECTRUM_BLOCK ? samples - first : (size_t)GDG_SPECTRUM_BLOCK);
    const double *x = rows + (size_t)row * row_stride + first;

    /* pass 0 straight from global memory: packed element e = (w[2e] x[2e], w[2e+1] x[2e+1]) */
    cplx v[16];
#pragma unroll
    for (int b = 0; b < B0; b++) {
        const int j = tid + T * b;
#pragma unroll
        for (int t = 0; t < R0; t++) {
            const int i = 2 * (j + t * (N / R0));
            double a = 0.0, c = 0.0;
            if (VEC && i + 1 < L) {
                const cplx q = gload(reinterpret_cast<const cplx *>(x + i));
                a = q.x;
                c = q.y;
            } else {
                if (i < L) a = gload1(x + i);
                if (i + 1 < L) c = gload1(x + i + 1);
            }
            const cplx w = gload(reinterpret_cast<const cplx *>(win + i));
            v[b * R0 + t] = make_double2(__dmul_rn(w.x, spectrum_finite(a)), __dmul_rn(w.y, spectrum_finite(c)));
        }
    }
    pass_compute<LOGN, LR0, 0, false>(v, tw, tid);
    pass_store<LOGN, LR0, 0>(v, sre, sim, tid);
    __syncthreads();
    run_lds_passes<LOGN, 1, sched_npass(LOGN), false>(v, sre, sim, tw, tid);

    /* un-pack Z -> X[k], X[N - k] (Z in natural order in LDS); c_k |X|^2 takes Z's place in sre: bins k and N - k belong to this thread alone */
#pragma unroll
    for (int i = 0; i < ITER; i++) {
        const int k = tid + T * i;
        if (k == 0) {
            const double zx = sre[0], zy = sim[0];
            const double x0 = zx + zy, xn = zx - zy;                                            /* X[0] and X[N] (Nyquist): real, c = 1 */
            const cplx xh = make_double2(sre[GDG_PAD(N / 2)], -sim[GDG_PAD(N / 2)]);
            sre[0] = __dmul_rn(x0, x0);
            sre[GDG_PAD(N)] = __dmul_rn(xn, xn);
            sre[GDG_PAD(N / 2)] = __dmul_rn(2.0, spectrum_sq(xh));
        } else {
            const int n = N - k;
            const cplx zk = make_double2(sre[GDG_PAD(k)], sim[GDG_PAD(k)]), zn = make_double2(sre[GDG_PAD(n)], sim[GDG_PAD(n)]);
            const cplx A = make_double2(zk.x + zn.x, zk.y - zn.y), Bv = make_double2(zk.x - zn.x, zk.y + zn.y);
            const cplx cw = cmul(tw2[k], Bv);
            const cplx ak = make_double2((A.x + cw.y) * 0.5, (A.y - cw.x) * 0.5), an = make_double2((A.x - cw.y) * 0.5, (-A.y - cw.x) * 0.5);
            sre[GDG_PAD(k)] = __dmul_rn(2.0, spectrum_sq(ak));
            sre[GDG_PAD(n)] = __dmul_rn(2.0, spectrum_sq(an));
        }
    }
    __syncthreads();

    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    double *dst = out + ((size_t)row * blocks_per_row + blockIdx.x) * (size_t)bands.n_bands;
    for (int b = wave; b < bands.n_bands; b += T / 64) {
        const int lo = bands.k_lo[b], hi = bands.k_lo[b + 1];
        double acc = 0.0;
        for (int k = lo + lane; k < hi; k += 64) acc = __dadd_rn(acc, sre[GDG_PAD(k)]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc = __dadd_rn(acc, __shfl_down(acc, o));
        if (lane == 0) gstore1(dst + b, acc / SPECTRUM_SCALE);
    }
}

/* d_bands: [n_rows][ceil(samples / 8192)][n_bands]; win: the 8192 window weights; tw, tw2: the tables of the 4096-point transform */
hipError_t gdg_launch_block_spectrum(const double *d_rows, size_t row_stride, unsigned n_rows, size_t samples, const double *d_win, const cplx *tw4096,
                                     const cplx *tw2_4096, const gdg_spectrum_bands &bands, double *d_bands, hipStream_t s) {
    if (n_rows == 0 || samples == 0) return hipSuccess;
    const size_t blocks = (samples + GDG_SPECTRUM_BLOCK - 1) / GDG_SPECTRUM_BLOCK;
    if (bands.n_bands < 1 || bands.n_bands >= GDG_SPECTRUM_MAX_EDGES) return hipErrorInvalidValue;
    for (int b = 0; b <= bands.n_bands; b++)
        if (bands.k_lo[b] < 0 || bands.k_lo[b] > GDG_SPECTRUM_BINS || (b && bands.k_lo[b] < bands.k_lo[b - 1])) return hipErrorInvalidValue;
    if (row_stride < samples || blocks > 0x7fffffffu || ((uintptr_t)d_rows & 7) || ((uintptr_t)d_bands & 7) || ((uintptr_t)d_win & 15)) return hipErrorInvalidValue;
    const bool vec = !((uintptr_t)d_rows & 15) && !(row_stride & 1);
    for (unsigned r0 = 0; r0 < n_rows; r0 += 65535u) {                      /* gridDim.y holds 65535 rows */
        const dim3 grid((unsigned)blocks, n_rows - r0 < 65535u ? n_rows - r0 : 65535u);
        if (vec) block_spectrum_kernel<true><<<grid, dim3(FftCfg<SPECTRUM_LOGN>::T), 0, s>>>(d_rows, row_stride, samples, r0, (unsigned)blocks, d_win, tw4096, tw2_4096, bands, d_bands);
        else block_spectrum_kernel<false><<<grid, dim3(FftCfg<SPECTRUM_LOGN>::T), 0, s>>>(d_rows, row_stride, samples, r0, (unsigned)blocks, d_win, tw4096, tw2_4096, bands, d_bands);
    }
    return hipGetLastError();
}
