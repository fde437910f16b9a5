/*
 * transfer_kernels.h -- the transfer records (include/gdg.h, TRANSFER, gdg_block_transfer_rows): per block of 8192 samples and
 * per (port, target) pair the two auto-spectra and the complex cross-spectrum, summed over groups of D bins.  No reference counterpart.
 * Included at the end of fir.hip, next to align_kernels.h and for its reason -- the register/LDS Stockham passes are defined there -- and in
 * front of the tuner's pragma: compiled without contraction, every product and every add below is rounded on its own.
 *
 * One workgroup of 512 threads per (block, pair): blockIdx.x = block (behind block0: a launch carries at most 65535), blockIdx.y = pair.
 * The windowed x (the port's block) and y (the target's) are the real and the imaginary part of ONE 8192-point complex transform
 * (FftCfg<13>: 16 points per thread, 136.25 KiB of LDS, one workgroup per CU):
 *   Z = F(w x + i w y);  A = Z[k] + conj Z[N-k] = 2 X[k],  B = Z[k] - conj Z[N-k] = 2i Y[k];  X = A / 2, Y = (B.y, -B.x) / 2.
 * THE WINDOW comes from the transform's own twiddle table: tw[n].x IS cos(2 pi n / 8192), rounded once from long double on the host, so
 * w[n] = 0.5 - 0.5 tw[n].x costs one cached load per sample and no cos() -- 16 of them per thread would cost more than the transform --
 * and needs no second table, upload or context field.
 * LEVELS: the largest |w x| and the largest |w y| of the block (fmax: exact, whatever the order) give each side a power of two of its own
 * that brings it below 2 before the two share a transform; the four values of a bin are scaled back by the same powers, exactly.  A side
 * whose windowed samples are all zero is silent: its transform is never looked at, every entry that involves it is +0.0.
 * Pxx, Pyy, Re Pxy, Im Pxy of bin k replace Z[k] and Z[N-k] in LDS (a thread writes only the entries it alone has read; bins 0 and 4096 are
 * their own partners, their imaginary part is +0.0 and their real cross part lies in the spare entries behind the data).  Then a thread owns
 * whole groups g = tid, tid + 512 ..: it adds the group's bins in ascending k into four running sums started at +0.0 and stores them with
 * two 16-byte stores (four 8-byte ones where the records are only 8-byte aligned).  D <= 64: no sum crosses threads; no atomics.  The order
 * is a function of D alone.  VEC reads a pair of samples with one 16-byte load where the launcher has seen that every block starts 16-byte
 * aligned; the values are the scalar path's.  A sample is read only when it lies inside the block: nothing outside [row, row + samples); a
 * short last block is zero-padded in registers.
 */
#include "blend.h"                                /* GDG_TRANSFER_BLOCK, _MAX_PAIRS, _MAX_GROUP: stated there for the code without include/gdg.h */
#define TRANSFER_LOGN 13
#define TRANSFER_SCALE 25165824.0                 /* L^2 * 3/8, L = 8192: the band spectrum's */

/* the exponent of a positive double, kept where 2^e and 2^-e are both normal doubles; a subnormal counts as 2^-1022 */
__device__ __forceinline__ int transfer_exp(double m) {
    const int e = (int)((__double_as_longlong(m) >> 52) & 0x7ff) - 1023;
    return e < -1022 ? -1022 : (e > 1022 ? 1022 : e);
}
__device__ __forceinline__ double transfer_pow2(int e) { return __longlong_as_double((long long)(1023 + e) << 52); }

template <bool VEC>
__global__ void __launch_bounds__(FftCfg<TRANSFER_LOGN>::T)
block_transfer_kernel(const double *__restrict__ rows, size_t row_stride, size_t samples, unsigned block0, const int *__restrict__ table, int group,
                      const cplx *__restrict__ tw, double *__restrict__ out, int out16) {
    constexpr int LOGN = TRANSFER_LOGN, N = FftCfg<LOGN>::N, T = FftCfg<LOGN>::T, NW = T / 64, H = N / 2;
    static_assert(N == GDG_TRANSFER_BLOCK && N / T == 16, "a block is one transform; sixteen samples per thread");
    __shared__ double s_all[2 * FftCfg<LOGN>::LDS];
    double *sre = s_all, *sim = s_all + FftCfg<LOGN>::LDS;
    /* the 16 entries the padded layout leaves free behind the last point: GDG_PAD(N - 1) < SPARE */
    constexpr int SPARE = FftCfg<LOGN>::LDS - 16;
    static_assert(GDG_PAD(N - 1) < SPARE && NW <= 16, "the spare entries lie behind the data");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned n_pairs = gridDim.y, pair = blockIdx.y;
    const size_t block = (size_t)block0 + blockIdx.x;
    const size_t row_x = (size_t)table[2 * pair], row_y = (size_t)table[2 * pair + 1];
    const size_t first = block * GDG_TRANSFER_BLOCK;
    const int L = (int)(samples - first < (size_t)GDG_TRANSFER_BLOCK ? samples - first : (size_t)GDG_TRANSFER_BLOCK);
    const double *x = rows + row_x * row_stride + first, *y = rows + row_y * row_stride + first;
    const int D = group, G = H / D + 1;
    double *rec = out + (block * n_pairs + pair) * (size_t)G * 4;
    auto store4 = [&](int g, double s0, double s1, double s2, double s3) {
        double *dst = rec + (size_t)g * 4;
        if (out16) {
            gstore(reinterpret_cast<cplx *>(dst), make_double2(s0, s1));
            gstore(reinterpret_cast<cplx *>(dst + 2), make_double2(s2, s3));
        } else {
            gstore1(dst + 0, s0); gstore1(dst + 1, s1); gstore1(dst + 2, s2); gstore1(dst + 3, s3);
        }
    };

    /* the two blocks, pair by pair and windowed: w x and w y in registers, their largest magnitudes on the way */
    double ax[N / T], cy[N / T];
    double mx = 0.0, my = 0.0;
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
        const double w0 = 0.5 - 0.5 * gload(tw + i).x, w1 = 0.5 - 0.5 * gload(tw + i + 1).x;
        a0 = w0 * spectrum_finite(a0);
        a1 = w1 * spectrum_finite(a1);
        c0 = w0 * spectrum_finite(c0);
        c1 = w1 * spectrum_finite(c1);
        mx = fmax(mx, fmax(fabs(a0), fabs(a1)));
        my = fmax(my, fmax(fabs(c0), fabs(c1)));
        ax[2 * t] = a0; ax[2 * t + 1] = a1; cy[2 * t] = c0; cy[2 * t + 1] = c1;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mx = fmax(mx, __shfl_down(mx, o));
        my = fmax(my, __shfl_down(my, o));
    }
    if (lane == 0) { sre[SPARE + wave] = mx; sim[SPARE + wave] = my; }
    __syncthreads();
    mx = sre[SPARE];
    my = sim[SPARE];
#pragma unroll
    for (int w = 1; w < NW; w++) { mx = fmax(mx, sre[SPARE + w]); my = fmax(my, sim[SPARE + w]); }     /* the same on every thread */

    const bool x_on = mx > 0.0, y_on = my > 0.0;
    if (!x_on && !y_on) {                                    /* both sides silent: the record is +0.0, and no transform runs */
        for (int g = tid; g < G; g += T) store4(g, 0.0, 0.0, 0.0, 0.0);
        return;
    }
    const int ex = x_on ? transfer_exp(mx) : 0, ey = y_on ? transfer_exp(my) : 0;
    {
        const double sx = transfer_pow2(-ex), sy = transfer_pow2(-ey);
#pragma unroll
        for (int t = 0; t < N / (2 * T); t++) {
            const int i = 2 * (tid + T * t);
            sre[GDG_PAD(i)] = x_on ? ax[2 * t] * sx : 0.0;
            sre[GDG_PAD(i + 1)] = x_on ? ax[2 * t + 1] * sx : 0.0;
            sim[GDG_PAD(i)] = y_on ? cy[2 * t] * sy : 0.0;
            sim[GDG_PAD(i + 1)] = y_on ? cy[2 * t + 1] * sy : 0.0;
        }
    }
    __syncthreads();
    cplx v[16];
    run_lds_passes<LOGN, 0, sched_npass(LOGN), false>(v, sre, sim, tw, tid);

    /* Z -> the bin's four values in place.  The powers of two go back on one factor at a time: 2^(2 ex) need not be a double where 2^ex is */
    const double bx = transfer_pow2(ex), by = transfer_pow2(ey);
    auto bin = [&](int k, int n) {
        const cplx zk = make_double2(sre[GDG_PAD(k)], sim[GDG_PAD(k)]), zn = make_double2(sre[GDG_PAD(n)], sim[GDG_PAD(n)]);
        const double xr = 0.5 * (zk.x + zn.x), xi = 0.5 * (zk.y - zn.y);              /* X[k] = A / 2 */
        const double yr = 0.5 * (zk.y + zn.y), yi = -0.5 * (zk.x - zn.x);             /* Y[k] = B / 2i */
        double pxx = (xr * xr + xi * xi) / TRANSFER_SCALE * bx * bx;
        double pyy = (yr * yr + yi * yi) / TRANSFER_SCALE * by * by;
        double pre = (xr * yr + xi * yi) / TRANSFER_SCALE * bx * by;                  /* conj X . Y */
        double pim = (xr * yi - xi * yr) / TRANSFER_SCALE * bx * by;
        if (!x_on) pxx = 0.0;
        if (!y_on) pyy = 0.0;
        if (!x_on || !y_on) { pre = 0.0; pim = 0.0; }
        sre[GDG_PAD(k)] = pxx;
        sim[GDG_PAD(k)] = pyy;
        if (n != k) { sre[GDG_PAD(n)] = pre; sim[GDG_PAD(n)] = pim; }
        else if (k == 0) sre[SPARE] = pre;                   /* X[0], Y[0], X[4096], Y[4096] are real: no imaginary cross part */
        else sim[SPARE] = pre;
    };
#pragma unroll
    for (int i = 0; i < H / T; i++) {
        const int k = tid + T * i;
        bin(k, (N - k) & (N - 1));
        if (k == 0) bin(H, H);
    }
    __syncthreads();

    /* the groups: bins g D - (D - 1) / 2 .. g D + D / 2, clipped to 0 .. 4096, ascending */
    for (int g = tid; g < G; g += T) {
        int lo = g * D - (D - 1) / 2, hi = g * D + D / 2;
        lo = lo < 0 ? 0 : lo;
        hi = hi > H ? H : hi;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        for (int k = lo; k <= hi; k++) {
            s0 = s0 + sre[GDG_PAD(k)];
            s1 = s1 + sim[GDG_PAD(k)];
            if (k == 0) s2 = s2 + sre[SPARE];
            else if (k == H) s2 = s2 + sim[SPARE];
            else { s2 = s2 + sre[GDG_PAD(N - k)]; s3 = s3 + sim[GDG_PAD(N - k)]; }
        }
        store4(g, s0, s1, s2, s3);
    }
}

/* d_records: [ceil(samples / 8192)][n_pairs][4096 / D + 1][4] doubles.  The table is port, target per pair and the group width D behind
 * them (blend.h, gdg_transfer_table): h_table is the host's copy of the device's d_table, held whole against the limits and n_rows before
 * anything is launched.  tw: the table of the 8192-point transform.  Row r at d_rows + r * row_stride. */
hipError_t gdg_launch_block_transfer(const double *d_rows, size_t row_stride, unsigned n_rows, size_t samples, const int *h_table, const int *d_table,
                                     unsigned n_pairs, const cplx *tw8192, void *d_records, hipStream_t s) {
    if (n_pairs == 0 || samples == 0) return hipSuccess;
    if (n_pairs > GDG_TRANSFER_MAX_PAIRS || !h_table || !d_table || !tw8192) return hipErrorInvalidValue;
    const int D = h_table[2 * n_pairs];
    if (D < 1 || D > GDG_TRANSFER_MAX_GROUP || (D & (D - 1))) return hipErrorInvalidValue;
    for (unsigned i = 0; i < 2 * n_pairs; i++)
        if (h_table[i] < 0 || (unsigned)h_table[i] >= n_rows) return hipErrorInvalidValue;
    const size_t blocks = (samples + GDG_TRANSFER_BLOCK - 1) / GDG_TRANSFER_BLOCK;
    if (row_stride < samples || blocks > 0x7fffffffu || ((uintptr_t)d_rows & 7) || ((uintptr_t)d_records & 7)) return hipErrorInvalidValue;
    const bool vec = !((uintptr_t)d_rows & 15) && !(row_stride & 1);
    const int out16 = !((uintptr_t)d_records & 15);              /* a group is 32 bytes: every group of every record is then 16-byte aligned */
    double *out = static_cast<double *>(d_records);
    for (size_t b0 = 0; b0 < blocks; b0 += 65535u) {             /* a launch holds 65535 blocks */
        const dim3 grid((unsigned)(blocks - b0 < 65535u ? blocks - b0 : 65535u), n_pairs);
        if (vec) block_transfer_kernel<true><<<grid, dim3(FftCfg<TRANSFER_LOGN>::T), 0, s>>>(d_rows, row_stride, samples, (unsigned)b0, d_table, D, tw8192, out, out16);
        else block_transfer_kernel<false><<<grid, dim3(FftCfg<TRANSFER_LOGN>::T), 0, s>>>(d_rows, row_stride, samples, (unsigned)b0, d_table, D, tw8192, out, out16);
    }
    return hipGetLastError();
}
