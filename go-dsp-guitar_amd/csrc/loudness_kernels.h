/*
 * loudness_kernels.h -- the loudness records (include/gdg.h, LOUDNESS): per port and 100 ms hop the sum of squares of the
 * K-weighted samples.  Included by loudness.hip and compiled without contraction; every product and sum below is rounded on its own.
 *
 * block_loudness_kernel: one workgroup of 256 threads per port (blockIdx.x = port), which walks the launch's tiles in order -- no port waits
 * on another.  The launch's samples are the job's [first, first + count), `first` a multiple of 8192: a tile is a block of 8192 samples counted
 * from the job's start (the last one of a stand-alone call may be short).  Per tile:
 *   - the tile is staged in LDS, 16 pairs a thread, their loads in flight together (a pair per 16-byte load where the launcher has seen that the
 *     rows allow it, two 8-byte loads otherwise); non-finite samples are zeroed on the way in, samples behind the launch's end are +0.0.  Chunk
 *     c of 32 samples lies at s_x[33 c ..]: thread t reads chunk t, 33 doubles apart, every bank once per half wave.
 *   - pass 1: thread t runs chunk t's recurrence in registers from state 0 (thread 0: from the tile's true incoming state) and keeps the state
 *     it ends with, f_t.
 *   - the scan: v_t = f_t, then for k = 0 .. 7  v_t = P[k] v_(t - 2^k) + v_t  where t >= 2^k  (P[k] = A^(32 * 2^k), uniform; through LDS, two
 *     buffers in turn, one barrier a level).  The structure is fixed, so v_t has the same bits in every launch.  Chunk t's true incoming state
 *     is v_(t - 1); the tile's outgoing state is v_255 -- of a short last tile, too: its chunks behind the end ran on +0.0.
 *   - pass 2: thread t runs its chunk again from the true incoming state and writes the squares of the outputs over its samples in LDS.
 *   - the sums: hop h of the job is the samples [h H, (h + 1) H), H = rate / 10; its cells are 64 samples counted from the hop's start, the last
 *     one shorter where 64 does not divide H.  Thread i sums the i-th cell that begins or continues in the tile, sequentially in sample order
 *     from +0.0 (thread 0: from the open cell's sum carried in); at most 152 cells at the rates the records are defined at.  Thread 0 then adds the complete cells to the open
 *     hop's sum in ascending order; a hop that ends leaves as one 8-byte vector store from that thread.  A cell the tile's end cuts stays the open cell.
 * The state (7 doubles a port) is read at the start and written at the end of the launch.  No atomics, no scratch.
 */
#include "loudness.h"

#define LOUDNESS_T 256
#define LOUDNESS_PITCH (LOUDNESS_CHUNK + 1)
#define LOUDNESS_MAX_CELLS LOUDNESS_T              /* a rate of 8000 or more: at most 12 hops touch a tile, each with two cells the tile's 128 do not count */

static_assert(LOUDNESS_T == LOUDNESS_CHUNKS, "a thread per chunk");
static_assert(LOUDNESS_T >= LOUDNESS_MAX_CELLS, "a thread per cell");
static_assert((1 << LOUDNESS_LEVELS) == LOUDNESS_T, "the scan's last distance is half the tile's chunks");

typedef double loud_v2d __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double loud_finite(double x) { return fabs(x) <= 1.7976931348623157e308 ? x : 0.0; }     /* NaN, +-inf: 0 */

/* one sample through both stages (include/gdg.h states the recurrence); s = (s0, s1, q0, q1) */
__device__ __forceinline__ double loud_step(const gdg_loudness_params &c, double s[4], double x) {
    const double y1 = __dadd_rn(__dmul_rn(c.shelf[0], x), s[0]);
    s[0] = __dadd_rn(__dsub_rn(__dmul_rn(c.shelf[1], x), __dmul_rn(c.shelf[3], y1)), s[1]);
    s[1] = __dsub_rn(__dmul_rn(c.shelf[2], x), __dmul_rn(c.shelf[4], y1));
    const double y2 = __dadd_rn(y1, s[2]);
    s[2] = __dadd_rn(s[2], __dsub_rn(s[3], __dmul_rn(c.beta, y2)));
    s[3] = __dsub_rn(s[3], __dmul_rn(c.alpha, y2));
    return y2;
}

extern "C" __global__ void __launch_bounds__(LOUDNESS_T)
block_loudness_kernel(const double *__restrict__ rows, size_t row_stride, unsigned long long first, unsigned long long count, unsigned long long hop, unsigned long long hop_base,
                      unsigned long long hops_room, const gdg_loudness_params par, double *__restrict__ state, double *__restrict__ records, int vec) {
    constexpr int T = LOUDNESS_T, C = LOUDNESS_CHUNK, PITCH = LOUDNESS_PITCH, ROUNDS = LOUDNESS_TILE / (2 * T);
    __shared__ double s_x[LOUDNESS_CHUNKS * LOUDNESS_PITCH];
    __shared__ double s_v[2][LOUDNESS_T][4];
    __shared__ double s_cell[LOUDNESS_MAX_CELLS];
    const int tid = (int)threadIdx.x;
    const unsigned port = blockIdx.x;
    const double *x_row = rows + (size_t)port * row_stride;
    double *st = state + (size_t)port * LOUDNESS_STATE;
    double *rec = records + (size_t)port * hops_room;
    const unsigned long long cells_per_hop = (hop + LOUDNESS_CELL - 1) / LOUDNESS_CELL;

    /* the tile's incoming state: every thread holds it, thread 0 runs from it */
    double in[4] = { st[0], st[1], st[2], st[3] };
    double cell_open = st[4], hop_open = st[5];

    for (unsigned long long t0 = 0; t0 < count; t0 += LOUDNESS_TILE) {
        const int TL = count - t0 < (unsigned long long)LOUDNESS_TILE ? (int)(count - t0) : LOUDNESS_TILE;
        const double *x = x_row + t0;
        double v[ROUNDS][2];
#pragma unroll
        for (int k = 0; k < ROUNDS; k++) {
            const int i = 2 * (k * T + tid);
            v[k][0] = v[k][1] = 0.0;
            if (vec && i + 1 < TL) {
                const loud_v2d q = *reinterpret_cast<const loud_v2d *>(x + i);
                v[k][0] = q.x;
                v[k][1] = q.y;
            } else {
                if (i < TL) v[k][0] = x[i];
                if (i + 1 < TL) v[k][1] = x[i + 1];
            }
        }
#pragma unroll
        for (int k = 0; k < ROUNDS; k++) {
            const int i = 2 * (k * T + tid), at = (i / C) * PITCH + (i % C);
            s_x[at] = loud_finite(v[k][0]);
            s_x[at + 1] = loud_finite(v[k][1]);
        }
        __syncthreads();

        /* pass 1: the chunk from state 0 -- thread 0 from the tile's incoming state */
        double xs[C];
#pragma unroll
        for (int j = 0; j < C; j++) xs[j] = s_x[tid * PITCH + j];
        double s[4] = { 0.0, 0.0, 0.0, 0.0 };
        if (tid == 0) { s[0] = in[0]; s[1] = in[1]; s[2] = in[2]; s[3] = in[3]; }
#pragma unroll
        for (int j = 0; j < C; j++) (void)loud_step(par, s, xs[j]);

        /* the scan of fixed structure over the 256 chunks */
        int cur = 0;
        s_v[0][tid][0] = s[0]; s_v[0][tid][1] = s[1]; s_v[0][tid][2] = s[2]; s_v[0][tid][3] = s[3];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < LOUDNESS_LEVELS; k++) {
            const int d = 1 << k;
            if (tid >= d) {
                const double u0 = s_v[cur][tid - d][0], u1 = s_v[cur][tid - d][1], u2 = s_v[cur][tid - d][2], u3 = s_v[cur][tid - d][3];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const double *m = par.P[k] + 4 * r;
                    const double acc = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(m[0], u0), __dmul_rn(m[1], u1)), __dmul_rn(m[2], u2)), __dmul_rn(m[3], u3));
                    s[r] = __dadd_rn(acc, s[r]);
                }
            }
            cur ^= 1;
            s_v[cur][tid][0] = s[0]; s_v[cur][tid][1] = s[1]; s_v[cur][tid][2] = s[2]; s_v[cur][tid][3] = s[3];
            __syncthreads();
        }
        /* the chunk's true incoming state, and the tile's outgoing one for every thread */
        if (tid > 0) { s[0] = s_v[cur][tid - 1][0]; s[1] = s_v[cur][tid - 1][1]; s[2] = s_v[cur][tid - 1][2]; s[3] = s_v[cur][tid - 1][3]; }
        else { s[0] = in[0]; s[1] = in[1]; s[2] = in[2]; s[3] = in[3]; }
        in[0] = s_v[cur][T - 1][0]; in[1] = s_v[cur][T - 1][1]; in[2] = s_v[cur][T - 1][2]; in[3] = s_v[cur][T - 1][3];

        /* pass 2: the chunk again from there; the squares replace its samples */
#pragma unroll
        for (int j = 0; j < C; j++) {
            const double y = loud_step(par, s, xs[j]);
            s_x[tid * PITCH + j] = __dmul_rn(y, y);
        }
        __syncthreads();

        /* the cells that begin or continue in the tile: cell g of the job is cell g % cells_per_hop of hop g / cells_per_hop */
        const unsigned long long a = first + t0, e = a + (unsigned long long)TL;
        const unsigned long long g0 = (a / hop) * cells_per_hop + (a % hop) / LOUDNESS_CELL;
        const unsigned long long g1 = ((e - 1) / hop) * cells_per_hop + ((e - 1) % hop) / LOUDNESS_CELL;
        const int n_cells = (int)(g1 - g0) + 1 < LOUDNESS_MAX_CELLS ? (int)(g1 - g0) + 1 : LOUDNESS_MAX_CELLS;
        if (tid < n_cells) {
            const unsigned long long g = g0 + (unsigned long long)tid, h = g / cells_per_hop, c = g % cells_per_hop;
            unsigned long long b0 = h * hop + c * LOUDNESS_CELL, b1 = b0 + LOUDNESS_CELL;
            if (b1 > (h + 1) * hop) b1 = (h + 1) * hop;
            if (b0 < a) b0 = a;
            if (b1 > e) b1 = e;
            double acc = tid == 0 ? cell_open : 0.0;
            for (int i = (int)(b0 - a); i < (int)(b1 - a); i++) acc = __dadd_rn(acc, s_x[(i / C) * PITCH + (i % C)]);
            s_cell[tid] = acc;
        }
        __syncthreads();
        if (tid == 0) {
            for (int i = 0; i < n_cells; i++) {
                const unsigned long long g = g0 + (unsigned long long)i, h = g / cells_per_hop, c = g % cells_per_hop;
                unsigned long long end = h * hop + (c + 1) * LOUDNESS_CELL;
                if (end > (h + 1) * hop) end = (h + 1) * hop;
                if (end > e) { cell_open = s_cell[i]; break; }                /* the tile's end cuts it: the next tile goes on */
                cell_open = 0.0;
                hop_open = __dadd_rn(hop_open, s_cell[i]);
                if (end == (h + 1) * hop) {
                    if (h >= hop_base && h - hop_base < hops_room) rec[h - hop_base] = hop_open;
                    hop_open = 0.0;
                }
            }
        }
        __syncthreads();                                                    /* the next tile overwrites what was just read */
    }
    if (tid == 0) {
        st[0] = in[0]; st[1] = in[1]; st[2] = in[2]; st[3] = in[3];
        st[4] = cell_open; st[5] = hop_open;
        st[6] = (double)(first + count);
    }
}

/* n_rows rows (row r at d_rows + r * row_stride, 8-byte aligned) hold the job's samples [first, first + count), `first` a multiple of 8192;
 * d_state: [n_rows][7], read and written; d_records: [n_rows][hops_room], hop h of the job at index h - hop_base. */
hipError_t gdg_launch_block_loudness(const double *d_rows, size_t row_stride, unsigned n_rows, unsigned long long first, unsigned long long count, uint32_t rate,
                                     unsigned long long hop_base, unsigned long long hops_room, const gdg_loudness_params &par, double *d_state, double *d_records, hipStream_t s) {
    if (n_rows == 0 || count == 0) return hipSuccess;
    if (!d_rows || !d_state || !d_records || row_stride < count || !gdg_loudness_rate_ok(rate) || first % LOUDNESS_TILE || ((uintptr_t)d_rows & 7) || ((uintptr_t)d_state & 7) ||
        ((uintptr_t)d_records & 7))
        return hipErrorInvalidValue;
    const bool vec = !((uintptr_t)d_rows & 15) && !(row_stride & 1);
    block_loudness_kernel<<<n_rows, LOUDNESS_T, 0, s>>>(d_rows, row_stride, first, count, gdg_loudness_hop(rate), hop_base, hops_room, par, d_state, d_records, vec ? 1 : 0);
    return hipGetLastError();
}
