/*
 * align_kernels.h -- the alignment report (include/gdg.h, gdg_block_align_rows): lag and polarity of a block of one output
 * row against the same block of a reference row.  No reference counterpart.  Included at the end of fir.hip, next to spectrum_kernels.h and
 * for its reason -- the register/LDS Stockham passes are defined there -- and in front of the tuner's pragma: compiled without contraction.
 *
 * One workgroup of 512 threads per (block, measured port): blockIdx.x = block, blockIdx.y = an entry of the pair list the launch carries in
 * its arguments.  x' (the reference block, zeroed outside its central [M, L - M)) and y (the port's block) are the real and the imaginary
 * part of ONE 8192-point complex transform (FftCfg<13>: 16 points per thread, 136.25 KiB of LDS, one workgroup per CU):
 *   Z = F(x' + i y);  2 X[k] = Z[k] + conj Z[N-k],  2i Y[k] = Z[k] - conj Z[N-k];  C[k] = conj X[k] Y[k] / N  replaces Z in place (a thread
 *   writes only the entries k and N - k it alone has read);  the inverse passes leave  r[l] = sum_n x'[n] y[n + l]  at entry l mod N.
 * x' is zero outside [M, L - M) and |l| <= M, so n + l stays inside the block: the circular correlation IS the linear one for every lag asked for.
 * The (|r|, lag) maximum over -M .. M: a thread walks the candidates tid, tid + 512 .. in ascending order, the 64 lanes meet in the tree
 * lane i <- lane i + 32, + 16 .. + 1, the 8 waves in wave order; "better" is lexicographic at every level -- greater |r|, then smaller |l|,
 * then the negative l -- so the result does not depend on the tree.  ref_sq is summed while the samples are loaded, sq_at_lag from a
 * second read of y once the lag is known: a thread adds its samples in ascending order, then the same two trees; every square
 * (__dmul_rn) and every add (align_add_sq, __dadd_rn in the trees) is rounded on its own, the order a function of M (and the lag) alone.
 * No atomics.  VEC reads a pair of samples with one 16-byte load where the launcher has seen that every block starts 16-byte aligned; the
 * values are the scalar path's.  A sample is read only when it lies inside the block: nothing outside [row, row + samples); a short last
 * block is zero-padded in registers.
 */
#define ALIGN_LOGN 13

__device__ __forceinline__ bool align_better(double ma, int la, double mb, int lb) {
    if (ma > mb) return true;
    if (!(ma == mb)) return false;
    const int aa = la < 0 ? -la : la, ab = lb < 0 ? -lb : lb;
    return aa < ab || (aa == ab && la < lb);
}

/* acc + v^2, the square and the add each rounded on its own.  __dmul_rn and __dadd_rn are inline functions of a header that is compiled with
 * contraction allowed: side by side they may fuse, and in one of this kernel's two variants they did (one bit of ref_sq).  The sum is
 * therefore written here, under the file's fp contract(off): an add that may not contract cannot take the product in */
__device__ __forceinline__ double align_add_sq(double acc, double v) { return acc + __dmul_rn(v, v); }

template <bool VEC>
__global__ void __launch_bounds__(FftCfg<ALIGN_LOGN>::T)
block_align_kernel(const double *__restrict__ rows, size_t row_stride, size_t samples, unsigned n_chain, unsigned tail_row, unsigned blocks_per_row,
                   const cplx *__restrict__ tw, gdg_align_pairs pairs, double *__restrict__ out) {
    constexpr int LOGN = ALIGN_LOGN, N = FftCfg<LOGN>::N, T = FftCfg<LOGN>::T, NW = T / 64;
    static_assert(N == GDG_ALIGN_BLOCK && 2 * GDG_ALIGN_MAX_LAG + 1 <= 9 * T && N / T == 16, "a block is one transform; nine candidates and sixteen samples per thread");
    __shared__ double s_all[2 * FftCfg<LOGN>::LDS];
    double *sre = s_all, *sim = s_all + FftCfg<LOGN>::LDS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = pairs.max_lag;
    const unsigned port = (unsigned)pairs.port[blockIdx.y], ref = (unsigned)pairs.ref[blockIdx.y];
    /* ports -> rows: the first n_chain ports are the rows of their number, the ports behind them the rows from tail_row on */
    const size_t row_x = ref < n_chain ? ref : ref - n_chain + tail_row, row_y = port < n_chain ? port : port - n_chain + tail_row;
    const size_t first = (size_t)blockIdx.x * GDG_ALIGN_BLOCK;
    const int L = (int)(samples - first < (size_t)GDG_ALIGN_BLOCK ? samples - first : (size_t)GDG_ALIGN_BLOCK);
    const double *x = rows + row_x * row_stride + first, *y = rows + row_y * row_stride + first;

    /* the two blocks, pair by pair: x' and y in registers, their energies on the way (ref_sq; the whole block of y) */
    double ax[N / T], cy[N / T];
    double ref_sq = 0.0, y_sq = 0.0;
#pragma unroll
    for (int t = 0; t < N / (2 * T); t++) {
        const int i = 2 * (tid + T * t);
        double a0 = 0.0, a1 = 0.0, c0 = 0.0, c1 = 0.0;
        if (VEC && i + 1 < L) {
            const cplx qa = gload(reinterpret_cast<const cplx *>(x + i)), qc = gload(reinterpret_cast<const cplx *>(y + i));
            a0 = qa.x; a1 = qa.y; c0 = qc.x; c1 = qc.y;
        } else {
            if (i < L) { a0 = gload1(x + i); c0 = gload1(y + i); }
            if (i + 1 < L) { a1 = gload1(x + i + 1); c1 = gload1(y + i + 1); }
        }
        a0 = (i >= M && i < N - M) ? spectrum_finite(a0) : 0.0;
        a1 = (i + 1 >= M && i + 1 < N - M) ? spectrum_finite(a1) : 0.0;
        c0 = spectrum_finite(c0);
        c1 = spectrum_finite(c1);
        ref_sq = align_add_sq(align_add_sq(ref_sq, a0), a1);
        y_sq = align_add_sq(align_add_sq(y_sq, c0), c1);
        ax[2 * t] = a0; ax[2 * t + 1] = a1; cy[2 * t] = c0; cy[2 * t + 1] = c1;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ref_sq = __dadd_rn(ref_sq, __shfl_down(ref_sq, o));
        y_sq = __dadd_rn(y_sq, __shfl_down(y_sq, o));
    }
    /* the waves' sums meet in the 16 entries the padded layout leaves free behind the last point: GDG_PAD(N - 1) < SPARE */
    constexpr int SPARE = FftCfg<LOGN>::LDS - 16;
    static_assert(GDG_PAD(N - 1) < SPARE && NW <= 16, "the spare entries lie behind the data");
    if (lane == 0) { sre[SPARE + wave] = ref_sq; sim[SPARE + wave] = y_sq; }
    __syncthreads();
    ref_sq = sre[SPARE];
    y_sq = sim[SPARE];
#pragma unroll
    for (int w = 1; w < NW; w++) { ref_sq = __dadd_rn(ref_sq, sre[SPARE + w]); y_sq = __dadd_rn(y_sq, sim[SPARE + w]); }     /* the same on every thread */

    /* A silent side: r is exactly zero, and no transform's rounding may say otherwise.  Otherwise both sides are brought to a size of
     * their own near 1 by a power of two (exact) before they share a transform -- its rounding is a few 1e-16 of |x'|^2 + |y|^2, which is
     * of the order of |x'| |y| only when the two are of one size -- and r is scaled back by the same powers. */
    const bool silent = !(ref_sq > 0.0) || !(y_sq > 0.0);
    int lag = 0;
    double corr = 0.0, corr0 = 0.0;
    if (!silent) {
        auto half_exp = [](double e) {                       /* floor(exponent / 2), kept where 2^(hx + hy) stays a double */
            int h = ((int)((__double_as_longlong(e) >> 52) & 0x7ff) - 1023) >> 1;
            return h < -480 ? -480 : (h > 480 ? 480 : h);
        };
        auto pow2 = [](int h) { return __longlong_as_double((long long)(1023 + h) << 52); };
        const int hx = half_exp(ref_sq), hy = half_exp(y_sq);
        const double sx = pow2(-hx), sy = pow2(-hy);
#pragma unroll
        for (int t = 0; t < N / (2 * T); t++) {
            const int i = 2 * (tid + T * t);
            sre[GDG_PAD(i)] = ax[2 * t] * sx;
            sre[GDG_PAD(i + 1)] = ax[2 * t + 1] * sx;
            sim[GDG_PAD(i)] = cy[2 * t] * sy;
            sim[GDG_PAD(i + 1)] = cy[2 * t + 1] * sy;
        }
        __syncthreads();
        cplx v[16];
        run_lds_passes<LOGN, 0, sched_npass(LOGN), false>(v, sre, sim, tw, tid);

        /* Z -> conj X . Y / N in place: with A = Z[k] + conj Z[n] = 2 X[k] and B = Z[k] - conj Z[n] = 2i Y[k], conj X Y = -i conj(A) B / 4;
         * entry n = N - k is its conjugate (both sequences are real).  k = 0 and k = N/2 are their own partners and the same formula holds */
        const double scale = (0.25 / (double)N) * pow2(hx + hy);
        auto combine = [&](int k, int n) {
            const cplx zk = make_double2(sre[GDG_PAD(k)], sim[GDG_PAD(k)]), zn = make_double2(sre[GDG_PAD(n)], sim[GDG_PAD(n)]);
            const cplx A = make_double2(zk.x + zn.x, zk.y - zn.y), Bv = make_double2(zk.x - zn.x, zk.y + zn.y);
            const double px = __builtin_fma(A.x, Bv.x, A.y * Bv.y), py = __builtin_fma(A.x, Bv.y, -(A.y * Bv.x));
            sre[GDG_PAD(k)] = py * scale;
            sim[GDG_PAD(k)] = -px * scale;
            if (n != k) {
                sre[GDG_PAD(n)] = py * scale;
                sim[GDG_PAD(n)] = px * scale;
            }
        };
#pragma unroll
        for (int i = 0; i < (N / 2) / T; i++) {
            const int k = tid + T * i;
            combine(k, (N - k) & (N - 1));
            if (k == 0) combine(N / 2, N / 2);
        }
        __syncthreads();
        run_lds_passes<LOGN, 0, sched_npass(LOGN), true>(v, sre, sim, tw, tid);

        /* r[l] is the real part at entry l mod N.  The maximum of |r| over -M .. M */
        double best = -1.0;
        int best_l = 0;
        for (int c = tid; c <= 2 * M; c += T) {
            const int l = c - M;
            const double m = fabs(sre[GDG_PAD(l & (N - 1))]);
            if (align_better(m, l, best, best_l)) { best = m; best_l = l; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double m = __shfl_down(best, o);
            const int l = __shfl_down(best_l, o);
            if (align_better(m, l, best, best_l)) { best = m; best_l = l; }
        }
        /* the imaginary parts (zero but for rounding) are not needed: their room carries the waves' results */
        if (lane == 0) { sim[wave] = best; sim[NW + wave] = (double)best_l; }
        __syncthreads();
        best = sim[0];
        best_l = (int)sim[NW];
#pragma unroll
        for (int w = 1; w < NW; w++)
            if (align_better(sim[w], (int)sim[NW + w], best, best_l)) { best = sim[w]; best_l = (int)sim[NW + w]; }
        lag = best_l;                                        /* the same on every thread */
        corr = sre[GDG_PAD(lag & (N - 1))];
        corr0 = sre[0];
    }

    /* sq_at_lag: the samples y[M + lag .. L - M + lag) that met the reference at this lag, read again (LDS and the registers are full) */
    double sq = 0.0;
#pragma unroll
    for (int t = 0; t < N / T; t++) {
        const int m = tid + T * t;
        double c = 0.0;
        if (m >= M + lag && m < N - M + lag && m < L) c = spectrum_finite(gload1(y + m));
        sq = align_add_sq(sq, c);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sq = __dadd_rn(sq, __shfl_down(sq, o));
    if (lane == 0) sim[2 * NW + wave] = sq;
    __syncthreads();
    if (tid == 0) {
        double s = sim[2 * NW];
#pragma unroll
        for (int w = 1; w < NW; w++) s = __dadd_rn(s, sim[2 * NW + w]);
        /* the record: corr, corr0, ref_sq, sq_at_lag, (lag, reserved = 0); x + 0.0 makes a -0.0 of the transform +0.0 */
        double *dst = out + ((size_t)port * blocks_per_row + blockIdx.x) * 5;
        gstore1(dst + 0, __dadd_rn(corr, 0.0));
        gstore1(dst + 1, __dadd_rn(corr0, 0.0));
        gstore1(dst + 2, ref_sq);
        gstore1(dst + 3, s);
        gstore1(dst + 4, __longlong_as_double((long long)(unsigned long long)(unsigned)lag));
    }
}

/* d_records: [ports][ceil(samples / 8192)] records of 40 bytes, of which the launch writes those of pairs.port[0 .. n); tw: the table of the
 * 8192-point transform.  Ports below n_chain are the rows of their number, the ports from n_chain on the rows from tail_row on; n_ports
 * bounds both columns of the list */
hipError_t gdg_launch_block_align(const double *d_rows, size_t row_stride, unsigned n_chain, unsigned tail_row, unsigned n_ports, size_t samples,
                                  const gdg_align_pairs &pairs, const cplx *tw8192, void *d_records, hipStream_t s) {
    if (pairs.n == 0 || samples == 0) return hipSuccess;
    const size_t blocks = (samples + GDG_ALIGN_BLOCK - 1) / GDG_ALIGN_BLOCK;
    if (pairs.n < 0 || pairs.n > GDG_ALIGN_PAIRS || pairs.max_lag < 1 || pairs.max_lag > GDG_ALIGN_MAX_LAG) return hipErrorInvalidValue;
    for (int i = 0; i < pairs.n; i++)
        if (pairs.port[i] < 0 || (unsigned)pairs.port[i] >= n_ports || pairs.ref[i] < 0 || (unsigned)pairs.ref[i] >= n_ports) return hipErrorInvalidValue;
    if (row_stride < samples || blocks > 0x7fffffffu || ((uintptr_t)d_rows & 7) || ((uintptr_t)d_records & 7) || !tw8192) return hipErrorInvalidValue;
    const bool vec = !((uintptr_t)d_rows & 15) && !(row_stride & 1);
    const dim3 grid((unsigned)blocks, (unsigned)pairs.n);
    double *out = static_cast<double *>(d_records);
    if (vec) block_align_kernel<true><<<grid, dim3(FftCfg<ALIGN_LOGN>::T), 0, s>>>(d_rows, row_stride, samples, n_chain, tail_row, (unsigned)blocks, tw8192, pairs, out);
    else block_align_kernel<false><<<grid, dim3(FftCfg<ALIGN_LOGN>::T), 0, s>>>(d_rows, row_stride, samples, n_chain, tail_row, (unsigned)blocks, tw8192, pairs, out);
    return hipGetLastError();
}
