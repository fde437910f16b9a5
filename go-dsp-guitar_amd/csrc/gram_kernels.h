/*
 * gram_kernels.h -- the Gram record (include/gdg.h, GRAM): per block the lower triangle of the P x P matrix of inner
 * products of P listed float64 rows, P up to 512 -- what a selection among many rigs needs, taken from the rows where they lie.  No
 * reference counterpart.  The first dense contraction of this code base, on the matrix cores: v_mfma_f64_16x16x4_f64 (tapfit_kernels.h is the second).
 * Included by gram.hip alone; contraction flags do not matter to it, the instruction is the arithmetic.
 *
 * blockIdx.x = a 64 x 64 tile of the lower triangle, diagonal tiles included, by rows: tile (ti, tj), tj <= ti, at ti (ti + 1) / 2 + tj;
 * blockIdx.y = the block (the launcher cuts more than 65535 blocks into launches).  A block's tiles are neighbours in dispatch order: they
 * read the same P rows of that block.  256 threads; wave w holds the 32 x 32 quarter (w >> 1, w & 1) as 2 x 2 accumulators of 4 doubles.
 *
 * ORDER OF THE SUM (normative, include/gdg.h): entry (i, j) is ONE accumulator element of one wave, and its value is the chain
 *     acc = +0.0;  for k = 0, 4, 8, ...:  acc = mfma(x_i[k .. k + 3], x_j[k .. k + 3], acc)
 * over the block's samples ascending, samples behind the block's end as +0.0.  k is never split over waves or workgroups, nothing is added
 * afterwards, and there are no atomics: the entry depends on the block's samples of its two rows alone -- not on P, on the positions in the
 * list, on the tile, on the chunk length below or on the grid.  (A chunk only says how many k lie in LDS at a time.)
 *
 * The two 64-row panels come through LDS in chunks of 32 samples.  A/B operand of the instruction: one double per lane, row lane & 15 at
 * k = lane >> 4; an LDS row has 34 doubles, so that the 16 rows x 2 k of a half-wave fall into 32 different 8-byte banks (34 = 2 mod 32).
 * C/D of the f64 form: col = lane & 15, row = (lane >> 4) + 4 * reg -- NOT the f32 forms' (lane >> 4) * 4 + reg.
 * The next chunk's global loads are issued before the current chunk's MFMAs and land in registers under them.  A diagonal tile has one
 * panel: it loads it once and reads it as both operands; it computes its square and stores j <= i.
 * Loads: thread t reads sample t & 31 of the chunk for the rows (t >> 5) + 8 m, m = 0 .. 7, of either panel -- 8-byte loads, a half-wave per
 * 256 contiguous bytes -- behind a guard: a row at or behind P and a sample at or behind the block's end are +0.0 and are NOT addressed;
 * nothing outside [row, row + samples) is.  Plain loads: the encoder and the other record kernels read the same rows.
 */
#define GRAM_T 256
#define GRAM_TILE 64
#define GRAM_KC 32                             /* samples per chunk */
#define GRAM_LDS_ROW 34                        /* doubles per LDS row: the chunk and 2 of padding */
#define GRAM_ROWS_PER_THREAD (GRAM_TILE * GRAM_KC / GRAM_T)
static_assert(GRAM_KC == 32 && GRAM_T == 256 && GRAM_ROWS_PER_THREAD == 8 && GRAM_KC % 4 == 0, "thread t loads sample t & 31 of rows (t >> 5) + 8 m");
static_assert(2 * GRAM_TILE * GRAM_LDS_ROW * sizeof(double) <= 80 * 1024, "two workgroups per CU");

typedef double gram_v4d __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(GRAM_T)
block_gram_kernel(const double *__restrict__ rows, size_t row_stride, size_t samples, unsigned block, unsigned block0, const int *__restrict__ ports, unsigned P,
                  double *__restrict__ records) {
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ double s_a[GRAM_TILE * GRAM_LDS_ROW], s_b[GRAM_TILE * GRAM_LDS_ROW];
    unsigned ti = 0;
    while ((ti + 1u) * (ti + 2u) / 2u <= blockIdx.x) ti++;
    const unsigned tj = blockIdx.x - ti * (ti + 1u) / 2u;
    const bool diag = ti == tj;                                              /* one value for the whole workgroup */
    const size_t q = (size_t)block0 + blockIdx.y;
    const size_t first = q * block;
    const unsigned L = (unsigned)(samples - first < (size_t)block ? samples - first : (size_t)block);
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, wr = wave >> 1, wc = wave & 1u;
    const unsigned lk = tid & (GRAM_KC - 1u), lr = tid / GRAM_KC;
    /* the rows this thread loads: null = a row at or behind P, never addressed */
    const double *pa[GRAM_ROWS_PER_THREAD], *pb[GRAM_ROWS_PER_THREAD];
#pragma unroll
    for (int m = 0; m < GRAM_ROWS_PER_THREAD; m++) {
        const unsigned ia = ti * GRAM_TILE + lr + 8u * m, ib = tj * GRAM_TILE + lr + 8u * m;
        pa[m] = ia < P ? rows + (size_t)(unsigned)ports[ia] * row_stride + first : nullptr;
        pb[m] = (!diag && ib < P) ? rows + (size_t)(unsigned)ports[ib] * row_stride + first : nullptr;
    }
    double va[GRAM_ROWS_PER_THREAD], vb[GRAM_ROWS_PER_THREAD];
    auto fetch = [&](unsigned k0) {
        const unsigned k = k0 + lk;
#pragma unroll
        for (int m = 0; m < GRAM_ROWS_PER_THREAD; m++) {
            va[m] = (pa[m] && k < L) ? pa[m][k] : 0.0;
            vb[m] = (pb[m] && k < L) ? pb[m][k] : 0.0;
        }
    };
    gram_v4d acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int n = 0; n < 2; n++) acc[m][n] = gram_v4d{ 0.0, 0.0, 0.0, 0.0 };
    const double *s_col = diag ? s_a : s_b;
    const unsigned a_at = (wr * 32u + (lane & 15u)) * GRAM_LDS_ROW + (lane >> 4), b_at = (wc * 32u + (lane & 15u)) * GRAM_LDS_ROW + (lane >> 4);
    fetch(0u);
    for (unsigned k0 = 0; k0 < L; k0 += GRAM_KC) {
#pragma unroll
        for (int m = 0; m < GRAM_ROWS_PER_THREAD; m++) {
            s_a[(lr + 8u * m) * GRAM_LDS_ROW + lk] = va[m];
            if (!diag) s_b[(lr + 8u * m) * GRAM_LDS_ROW + lk] = vb[m];
        }
        __syncthreads();
        if (k0 + GRAM_KC < L) fetch(k0 + GRAM_KC);                           /* in flight under the MFMAs below */
#pragma unroll
        for (unsigned k = 0; k < GRAM_KC; k += 4) {
            const double a0 = s_a[a_at + k], a1 = s_a[a_at + 16u * GRAM_LDS_ROW + k];
            const double b0 = s_col[b_at + k], b1 = s_col[b_at + 16u * GRAM_LDS_ROW + k];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
    /* the record: entry (i, j), j <= i, at i (i + 1) / 2 + j; 16 lanes write 16 neighbours of one row */
    double *rec = records + q * ((size_t)P * (P + 1u) / 2u);
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int n = 0; n < 2; n++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const unsigned i = ti * GRAM_TILE + wr * 32u + 16u * m + (lane >> 4) + 4u * r;
                const unsigned j = tj * GRAM_TILE + wc * 32u + 16u * n + (lane & 15u);
                if (i < P && j <= i) rec[(size_t)i * (i + 1u) / 2u + j] = acc[m][n][r];
            }
#endif
}

/* d_records: [ceil(samples / block)][P (P + 1) / 2] doubles.  h_ports is the host's copy of the P entries at d_ports, checked here against
 * n_rows (and for repeats) before anything is launched: the kernel reads rows by what the table says */
hipError_t gdg_launch_block_gram(const double *d_rows, size_t row_stride, unsigned n_rows, size_t samples, unsigned block, const int *h_ports, const int *d_ports,
                                 unsigned n_ports, void *d_records, hipStream_t s) {
    if (n_ports == 0 || samples == 0) return hipSuccess;
    if (block == 0 || n_ports > GDG_GRAM_MAX_PORTS || !h_ports || !d_ports || !d_rows || !d_records) return hipErrorInvalidValue;
    if (gdg_gram_list_bad(h_ports, (int)n_ports, (int)n_rows) >= 0) return hipErrorInvalidValue;
    const size_t blocks = (samples + block - 1) / block;
    if (row_stride < samples || blocks > 0x7fffffffu || ((uintptr_t)d_rows & 7) || ((uintptr_t)d_records & 7) || ((uintptr_t)d_ports & 3)) return hipErrorInvalidValue;
    const unsigned T = (n_ports + GRAM_TILE - 1) / GRAM_TILE;
    for (size_t b0 = 0; b0 < blocks; b0 += 65535u) {
        const unsigned n = (unsigned)(blocks - b0 < 65535u ? blocks - b0 : 65535u);
        block_gram_kernel<<<dim3(T * (T + 1u) / 2u, n), GRAM_T, 0, s>>>(d_rows, row_stride, samples, block, (unsigned)b0, d_ports, n_ports, static_cast<double *>(d_records));
    }
    return hipGetLastError();
}
