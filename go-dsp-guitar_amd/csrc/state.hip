/*
 * state.hip -- the one kernel behind gdg_state_save / gdg_state_load (api_state.cpp): a list of contiguous pieces {src, dst, bytes} moved
 * in one launch.  The host cuts a save or a load into one piece per state region (a unit's small state, its history ring, a power amp's
 * overlap-save history, every delay-line slot, a spatializer row), so the delay line's rotation into another ring size is only a matter of
 * addresses.  A piece without a source writes zeros (the stamps of the sums made ahead, padding in the blob).
 *
 * Memory bound and read once: 16-byte non-temporal loads through the global address space (a FLAT load would also count as an LDS
 * operation, fir.hip), plain 16-byte stores.  Every piece is cut into chunks of GDG_STATE_CHUNK bytes, a workgroup per chunk, found
 * through the prefix table `first` (first[i] = the first chunk of piece i).
 *
 * ... and the digest a checkpoint container carries over its payload (api_checkpoint.cpp): one pass of the same 16-byte loads, two 64-bit
 * multiplies per granule, a reduction per workgroup in LDS, one 16-byte store per workgroup; the host adds the partials up.
 */
#include "gdg_internal.h"

#define GDG_GLOBAL __attribute__((address_space(1)))
#define STATE_THREADS 256
#define STATE_V4 (GDG_STATE_CHUNK / 16 / STATE_THREADS)          /* 16-byte accesses per lane in a whole chunk */

typedef unsigned int v4u __attribute__((ext_vector_type(4)));
typedef unsigned int v2u __attribute__((ext_vector_type(2)));

template <typename T>
__device__ __forceinline__ T state_load(const char *p) {
    return __builtin_nontemporal_load(reinterpret_cast<const GDG_GLOBAL T *>((const GDG_GLOBAL void *)p));
}
template <typename T>
__device__ __forceinline__ void state_store(char *p, T v) {
    *reinterpret_cast<GDG_GLOBAL T *>((GDG_GLOBAL void *)p) = v;
}

/* bytes [from, to) of the piece in accesses of sizeof(T), `to - from` a multiple of it; src == nullptr: zeros */
template <typename T>
__device__ __forceinline__ void state_move(const char *src, char *dst, size_t from, size_t to) {
    for (size_t i = from + (size_t)threadIdx.x * sizeof(T); i < to; i += (size_t)STATE_THREADS * sizeof(T)) {
        T v = src ? state_load<T>(src + i) : T(0);
        state_store<T>(dst + i, v);
    }
}

__global__ __launch_bounds__(STATE_THREADS) void state_copy_kernel(const gdg_state_piece *__restrict__ pieces, const unsigned *__restrict__ first,
                                                                   int n_pieces) {
    const unsigned c = blockIdx.x;
    int lo = 0, hi = n_pieces - 1;                 /* the last piece whose first chunk is <= c */
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first[mid] <= c) lo = mid; else hi = mid - 1;
    }
    const gdg_state_piece p = pieces[lo];
    const size_t off = (size_t)(c - first[lo]) * GDG_STATE_CHUNK;
    if (off >= p.bytes) return;
    const size_t len = p.bytes - off < (size_t)GDG_STATE_CHUNK ? p.bytes - off : (size_t)GDG_STATE_CHUNK;
    const char *src = p.src ? static_cast<const char *>(p.src) + off : nullptr;
    char *dst = static_cast<char *>(p.dst) + off;
    const uintptr_t al = (uintptr_t)src | (uintptr_t)dst;          /* a chunk starts on a multiple of 16 of its piece: same alignment */
    size_t done = 0;
    if ((al & 15) == 0) {
        if (len == (size_t)GDG_STATE_CHUNK) {
            /* a whole chunk: every lane's loads in flight before its stores */
            v4u v[STATE_V4];
#pragma unroll
            for (int j = 0; j < STATE_V4; j++) {
                const size_t i = ((size_t)j * STATE_THREADS + threadIdx.x) * 16;
                v[j] = src ? state_load<v4u>(src + i) : v4u(0);
            }
#pragma unroll
            for (int j = 0; j < STATE_V4; j++) state_store<v4u>(dst + ((size_t)j * STATE_THREADS + threadIdx.x) * 16, v[j]);
            return;
        }
        done = len & ~(size_t)15;
        state_move<v4u>(src, dst, 0, done);
    }
    /* the tail (a ring of cp + 1 doubles), or a piece that is only 8- / 4-byte aligned (a spatializer row, the stamps) */
    if (((al | done) & 7) == 0) {
        const size_t end = done + ((len - done) & ~(size_t)7);
        state_move<v2u>(src, dst, done, end);
        done = end;
    }
    if (((al | done) & 3) == 0) {
        const size_t end = done + ((len - done) & ~(size_t)3);
        state_move<unsigned>(src, dst, done, end);
        done = end;
    }
    state_move<unsigned char>(src, dst, done, len);
}

hipError_t gdg_launch_state_copy(const gdg_state_piece *d_pieces, const unsigned *d_first, int n_pieces, unsigned n_chunks, hipStream_t s) {
    if (n_pieces <= 0 || n_chunks == 0) return hipSuccess;
    hipLaunchKernelGGL(state_copy_kernel, dim3(n_chunks), dim3(STATE_THREADS), 0, s, d_pieces, d_first, n_pieces);
    return hipGetLastError();
}

/* ---- the payload digest (gdg_internal.h states the function) ---------------------------------------------------------------------- */
#define DIGEST_V4 4                                              /* 16-byte loads a lane has in flight */

__global__ __launch_bounds__(STATE_THREADS) void state_digest_kernel(const char *__restrict__ payload, unsigned long long granules,
                                                                     unsigned long long *__restrict__ partials) {
    __shared__ unsigned long long red[2][STATE_THREADS];
    unsigned long long s0 = 0, s1 = 0;
    const unsigned long long round = (unsigned long long)STATE_THREADS * DIGEST_V4;
    for (unsigned long long base = (unsigned long long)blockIdx.x * round; base < granules; base += (unsigned long long)gridDim.x * round) {
        v4u w[DIGEST_V4];
#pragma unroll
        for (int j = 0; j < DIGEST_V4; j++) {
            const unsigned long long g = base + (unsigned long long)j * STATE_THREADS + threadIdx.x;
            w[j] = g < granules ? state_load<v4u>(payload + g * 16) : v4u(0);
        }
#pragma unroll
        for (int j = 0; j < DIGEST_V4; j++) {
            const unsigned long long g = base + (unsigned long long)j * STATE_THREADS + threadIdx.x;
            if (g >= granules) continue;
            const unsigned long long a = (unsigned long long)w[j].x | ((unsigned long long)w[j].y << 32);
            const unsigned long long b = (unsigned long long)w[j].z | ((unsigned long long)w[j].w << 32);
            unsigned long long u = (a + (g + 1) * GDG_DIGEST_K) * GDG_DIGEST_M0;
            u ^= u >> 32;
            unsigned long long v = (b ^ u) * GDG_DIGEST_M1;
            v ^= v >> 29;
            s0 += u;
            s1 ^= v;
        }
    }
    red[0][threadIdx.x] = s0;
    red[1][threadIdx.x] = s1;
    __syncthreads();
    for (int h = STATE_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            red[0][threadIdx.x] += red[0][threadIdx.x + h];
            red[1][threadIdx.x] ^= red[1][threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const unsigned long long t0 = red[0][0], t1 = red[1][0];
        v4u out = { (unsigned)t0, (unsigned)(t0 >> 32), (unsigned)t1, (unsigned)(t1 >> 32) };
        state_store<v4u>(reinterpret_cast<char *>(partials + 2 * (size_t)blockIdx.x), out);
    }
}

hipError_t gdg_launch_state_digest(const void *d_payload, unsigned long long granules, unsigned long long *d_partials, int groups, hipStream_t s) {
    if (granules == 0 || groups <= 0) return hipSuccess;
    hipLaunchKernelGGL(state_digest_kernel, dim3((unsigned)groups), dim3(STATE_THREADS), 0, s, static_cast<const char *>(d_payload), granules, d_partials);
    return hipGetLastError();
}
