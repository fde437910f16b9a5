/*
 * tapfit_kernels.h -- the tap-fit record (include/gdg.h, TAPFIT): per block and fit the lower triangle of the Gram matrix of
 * V = K T + 1 VIRTUAL rows -- term j at lag a, x[p_j][i - a], a = 0 .. T - 1, and the target at lag 0 -- over n = 0 .. L - T, i = first + T - 1
 * + n: the normal equations of "which T taps per term come closest to the target".  No reference counterpart.  Included by gram.hip alone,
 * behind gram_kernels.h, whose instruction, C/D layout and order of the sum it shares.
 *
 * The 64 lags of a term are NOT 64 rows: per chunk of TAPFIT_KC values of n every ACTUAL row a tile needs (at most K + 1 <= 5) is staged
 * once into LDS with a halo of T - 1 samples in front, and the MFMA operand of virtual row (j, a) at k is the LDS word at TAPFIT_HALO + k - a
 * of row j.  The 16 virtual rows of an operand are consecutive lags, so their words lie in consecutive 8-byte banks, and the second
 * sixteen lanes of a half-wave (k + 1) read 15 of the same addresses again, which broadcast.  An LDS row has TAPFIT_HALO + TAPFIT_KC = 192
 * doubles; where 16 virtual rows span two terms and T < 16 two of the addresses may share a bank (2-way, once per term border).
 *
 * blockIdx.x = a 32 x 32 tile of the lower triangle of one fit, diagonal tiles included, by rows, the fits' tiles behind one another in list
 * order (the table says where a fit's begin); blockIdx.y = the block (the launcher cuts more than 65535 blocks into launches).  256 threads;
 * wave w holds the 16 x 16 quarter (w >> 1, w & 1) in ONE accumulator of 4 doubles.  Small tiles on purpose: V <= 129, so a fit is at most
 * 15 tiles and the work per block is small -- the time is the length of the dependent MFMA chain, which a larger tile only multiplies
 * (the Gram kernel's 64-port case), and small tiles spread a step's few blocks over more CUs.
 *
 * ORDER OF THE SUM (normative, include/gdg.h): entry (u, v) is ONE accumulator element of one wave, and its value is the chain
 *     acc = +0.0;  for n = 0, 4, 8, ...:  acc = mfma(row_u[n .. n + 3], row_v[n .. n + 3], acc)
 * ascending, positions behind L - T as +0.0 in BOTH operands (the sample there may exist: it is a lag of a later n that does not).  n is
 * never split over waves or workgroups, nothing is added afterwards, no atomics.  This is block_gram_kernel's chain on the V shifted rows.
 * C/D of the f64 form: col = lane & 15, row = (lane >> 4) + 4 * reg (gram_kernels.h).
 *
 * The next chunk's global loads are issued before the current chunk's MFMAs and land in registers under them.  Loads: element e = t + 256 m,
 * m = 0 .. 3, of the [5][192] image is word x = e % 192 of staged row e / 192, which is sample first + n0 + x - TAPFIT_HALO + T - 1 of that
 * row -- plain 8-byte loads behind a guard: a staged row the tile does not need, a word in front of the halo and a sample at or behind the
 * block's end are +0.0 and are NOT addressed; nothing outside [row + first, row + first + L) is.
 */
#define TAPFIT_T 256
#define TAPFIT_TILE 32
#define TAPFIT_KC 128                          /* values of n per chunk */
#define TAPFIT_HALO 64                         /* doubles in front of a chunk: room for T - 1 <= 63 lags */
#define TAPFIT_LDS_ROW (TAPFIT_HALO + TAPFIT_KC)
#define TAPFIT_ROWS (GDG_TAPFIT_MAX_TERMS + 1) /* staged rows: the terms and the target */
#define TAPFIT_LOADS ((TAPFIT_ROWS * TAPFIT_LDS_ROW + TAPFIT_T - 1) / TAPFIT_T)
static_assert(TAPFIT_HALO >= GDG_BLEND_MAX_TAPS - 1 && TAPFIT_KC % 4 == 0 && TAPFIT_LOADS == 4 && TAPFIT_TILE == 32 && TAPFIT_T == 256, "4 waves of one 16 x 16 quarter; 4 loads per thread and chunk");

__global__ void __launch_bounds__(TAPFIT_T)
block_tapfit_kernel(const double *__restrict__ rows, size_t row_stride, size_t samples, unsigned block, unsigned block0, const int *__restrict__ table, unsigned n_fits,
                    size_t doubles_per_block, double *__restrict__ records) {
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ double s_x[TAPFIT_ROWS * TAPFIT_LDS_ROW];
    /* the fit of this tile: the last one whose tiles begin at or in front of blockIdx.x -- one value for the whole workgroup */
    unsigned f = 0;
    while (f + 1u < n_fits && (unsigned)table[(f + 1u) * GDG_TAPFIT_TABLE_INTS + TAPFIT_E_TILE0] <= blockIdx.x) f++;
    const int *fit = table + f * GDG_TAPFIT_TABLE_INTS;
    const unsigned K = (unsigned)fit[TAPFIT_E_TERMS], T = (unsigned)fit[TAPFIT_E_TAPS], U = K * T, V = U + 1u;
    const unsigned tile = blockIdx.x - (unsigned)fit[TAPFIT_E_TILE0];
    unsigned ti = 0;
    while ((ti + 1u) * (ti + 2u) / 2u <= tile) ti++;
    const unsigned tj = tile - ti * (ti + 1u) / 2u;
    const size_t q = (size_t)block0 + blockIdx.y;
    const size_t first = q * block;
    const unsigned L = (unsigned)(samples - first < (size_t)block ? samples - first : (size_t)block);
    const unsigned N = L >= T ? L - T + 1u : 0u;                             /* the positions n of this block */
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, wr = wave >> 1, wc = wave & 1u;
    /* staged row r: term r for r < K, the target at r == K.  The rows the two panels of this tile read: */
    auto staged_of = [&](unsigned v) { return v < U ? v / T : K; };
    unsigned need = 0u;
    {
        const unsigned a0 = ti * TAPFIT_TILE, a1 = (a0 + TAPFIT_TILE < V ? a0 + TAPFIT_TILE : V) - 1u;
        const unsigned b0 = tj * TAPFIT_TILE, b1 = (b0 + TAPFIT_TILE < V ? b0 + TAPFIT_TILE : V) - 1u;
        for (unsigned r = staged_of(a0); r <= staged_of(a1); r++) need |= 1u << r;
        for (unsigned r = staged_of(b0); r <= staged_of(b1); r++) need |= 1u << r;
    }
    /* what this thread loads: null = a staged row that does not exist or is not needed, or a word in front of the halo -- never addressed */
    const double *px[TAPFIT_LOADS];
    unsigned sx[TAPFIT_LOADS];                                               /* the sample of the block that word holds in chunk 0 */
#pragma unroll
    for (int m = 0; m < TAPFIT_LOADS; m++) {
        const unsigned e = tid + TAPFIT_T * m, r = e / TAPFIT_LDS_ROW, x = e % TAPFIT_LDS_ROW;
        const bool on = r <= K && ((need >> r) & 1u) && x + T - 1u >= TAPFIT_HALO;
        sx[m] = x + T - 1u - TAPFIT_HALO;
        px[m] = on ? rows + (size_t)(unsigned)fit[r < K ? TAPFIT_E_PORT + r : TAPFIT_E_TARGET] * row_stride + first : nullptr;
    }
    double vx[TAPFIT_LOADS];
    auto fetch = [&](unsigned n0) {
#pragma unroll
        for (int m = 0; m < TAPFIT_LOADS; m++) {
            const unsigned s = n0 + sx[m];
            vx[m] = (px[m] && s < L) ? px[m][s] : 0.0;
        }
    };
    /* the operands of this lane: virtual row u of the row panel, v of the column panel, at k = lane >> 4 of every group of four */
    const unsigned u = ti * TAPFIT_TILE + wr * 16u + (lane & 15u), v = tj * TAPFIT_TILE + wc * 16u + (lane & 15u), kq = lane >> 4;
    const bool u_on = u < V, v_on = v < V;
    const unsigned a_at = u_on ? staged_of(u) * TAPFIT_LDS_ROW + TAPFIT_HALO + kq - (u < U ? u % T : 0u) : 0u;
    const unsigned b_at = v_on ? staged_of(v) * TAPFIT_LDS_ROW + TAPFIT_HALO + kq - (v < U ? v % T : 0u) : 0u;
    gram_v4d acc = gram_v4d{ 0.0, 0.0, 0.0, 0.0 };
    fetch(0u);
    for (unsigned n0 = 0; n0 < N; n0 += TAPFIT_KC) {
#pragma unroll
        for (int m = 0; m < TAPFIT_LOADS; m++) {
            const unsigned e = tid + TAPFIT_T * m;
            if (e < TAPFIT_ROWS * TAPFIT_LDS_ROW) s_x[e] = vx[m];
        }
        __syncthreads();
        if (n0 + TAPFIT_KC < N) fetch(n0 + TAPFIT_KC);                       /* in flight under the MFMAs below */
        const unsigned left = N - n0;                                        /* positions from n0 on; k at or behind it is +0.0 */
#pragma unroll
        for (unsigned k = 0; k < TAPFIT_KC; k += 4) {
            const bool in = k + kq < left;
            const double a = (u_on && in) ? s_x[a_at + k] : 0.0;
            const double b = (v_on && in) ? s_x[b_at + k] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    /* the record: entry (i, j), j <= i, at i (i + 1) / 2 + j of the fit's part of the block's record; 16 lanes write 16 neighbours of one row */
    double *rec = records + q * doubles_per_block + (size_t)(unsigned)fit[TAPFIT_E_OFFSET];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const unsigned i = ti * TAPFIT_TILE + wr * 16u + (lane >> 4) + 4u * r;
        const unsigned j = tj * TAPFIT_TILE + wc * 16u + (lane & 15u);
        if (i < V && j <= i) rec[(size_t)i * (i + 1u) / 2u + j] = acc[r];
    }
#endif
}

/* d_records: [ceil(samples / block)][D] doubles, D the sum of the fits' V (V + 1) / 2.  h_table is the host's copy of the n_fits entries at
 * d_table (blend.h, gdg_tapfit_table), checked here -- limits, ports against n_rows, offsets and tiles against what the limits allow --
 * before anything is launched: the kernel reads rows and writes records by what the table says */
hipError_t gdg_launch_block_tapfit(const double *d_rows, size_t row_stride, unsigned n_rows, size_t samples, unsigned block, const int *h_table, const int *d_table,
                                   unsigned n_fits, void *d_records, hipStream_t s) {
    if (n_fits == 0 || samples == 0) return hipSuccess;
    if (block == 0 || n_fits > GDG_TAPFIT_MAX_FITS || !h_table || !d_table || !d_rows || !d_records) return hipErrorInvalidValue;
    unsigned tiles = 0;
    size_t D = 0;
    for (unsigned f = 0; f < n_fits; f++) {
        const int *e = h_table + (size_t)f * GDG_TAPFIT_TABLE_INTS;
        const int K = e[TAPFIT_E_TERMS], T = e[TAPFIT_E_TAPS];
        if (K < 1 || K > GDG_TAPFIT_MAX_TERMS || T < 1 || T > GDG_BLEND_MAX_TAPS || K * T > GDG_TAPFIT_MAX_UNKNOWNS) return hipErrorInvalidValue;
        if (e[TAPFIT_E_TARGET] < 0 || (unsigned)e[TAPFIT_E_TARGET] >= n_rows) return hipErrorInvalidValue;
        for (int k = 0; k < K; k++) if (e[TAPFIT_E_PORT + k] < 0 || (unsigned)e[TAPFIT_E_PORT + k] >= n_rows) return hipErrorInvalidValue;
        if ((size_t)e[TAPFIT_E_OFFSET] != D || (unsigned)e[TAPFIT_E_TILE0] != tiles) return hipErrorInvalidValue;
        const unsigned V = (unsigned)(K * T) + 1u, R = (V + TAPFIT_TILE - 1) / TAPFIT_TILE;
        D += (size_t)V * (V + 1u) / 2u;
        tiles += R * (R + 1u) / 2u;
    }
    const size_t blocks = (samples + block - 1) / block;
    if (row_stride < samples || blocks > 0x7fffffffu || ((uintptr_t)d_rows & 7) || ((uintptr_t)d_records & 7) || ((uintptr_t)d_table & 3)) return hipErrorInvalidValue;
    for (size_t b0 = 0; b0 < blocks; b0 += 65535u) {
        const unsigned n = (unsigned)(blocks - b0 < 65535u ? blocks - b0 : 65535u);
        block_tapfit_kernel<<<dim3(tiles, n), TAPFIT_T, 0, s>>>(d_rows, row_stride, samples, block, (unsigned)b0, d_table, n_fits, D, static_cast<double *>(d_records));
    }
    return hipGetLastError();
}
