/*
 * blend_kernels.h -- the blend outputs (include/gdg.h, gdg_batch_set_blends and gdg_blend_rows): row b of `out` is the
 * weighted sum of blend b's terms over the rows of `rows`, s = w_0 x[c_0] and then s = s + w_k x[c_k] in term order, every product and every
 * add rounded on its own (blend.h).  No reference counterpart; included by io.hip next to the record kernels and compiled like them without
 * contraction.
 *
 * blockIdx.y = the blend, blockIdx.x covers the live width.  A lane takes one 16-byte pair of samples where the launcher has seen that every
 * row of both sides starts 16-byte aligned (VEC), one 8-byte sample otherwise; a VEC launch's last lane takes the odd sample of an odd
 * width by the 8-byte path.  A lane reads and writes only inside [0, samples) of a row.  The term table -- first, channel, weight -- is
 * read at addresses that depend on blockIdx.y alone: uniform, fetched by scalar loads.  The term loop is unrolled by four: four row loads
 * are in flight before the first of their adds, and the adds stay in term order.  No LDS, no atomics, no scratch, and plain loads and stores
 * on both sides: the chain rows are read again by the encoder, the blend rows at once by the encoder and the record kernels.
 */
#define BLEND_T 256

template <typename T> struct blend_ops;
template <> struct blend_ops<double> {
    static __device__ __forceinline__ double mul(double w, double x) { return gdg_blend_mul(w, x); }
    static __device__ __forceinline__ double add(double s, double p) { return gdg_blend_add(s, p); }
};
template <> struct blend_ops<v2d> {
    static __device__ __forceinline__ v2d mul(double w, v2d x) { const v2d r = { gdg_blend_mul(w, x.x), gdg_blend_mul(w, x.y) }; return r; }
    static __device__ __forceinline__ v2d add(v2d s, v2d p) { const v2d r = { gdg_blend_add(s.x, p.x), gdg_blend_add(s.y, p.y) }; return r; }
};

/* the terms [k0, k1) at sample `at` of every row (T = v2d: the pair at, at + 1) */
template <typename T>
__device__ __forceinline__ void blend_terms(const double *rows, size_t row_stride, size_t at, const int *__restrict__ channel, const double *__restrict__ weight,
                                            int k0, int k1, double *dst) {
    typedef blend_ops<T> op;
    auto load = [&](int k) { return *reinterpret_cast<const T *>(rows + (size_t)channel[k] * row_stride + at); };
    int k = k0;
    T s = op::mul(weight[k], load(k));
    k++;
    for (; k + 4 <= k1; k += 4) {
        const T x0 = load(k), x1 = load(k + 1), x2 = load(k + 2), x3 = load(k + 3);
        s = op::add(s, op::mul(weight[k], x0));
        s = op::add(s, op::mul(weight[k + 1], x1));
        s = op::add(s, op::mul(weight[k + 2], x2));
        s = op::add(s, op::mul(weight[k + 3], x3));
    }
    for (; k < k1; k++) s = op::add(s, op::mul(weight[k], load(k)));
    *reinterpret_cast<T *>(dst + at) = s;
}

template <bool VEC>
__global__ void __launch_bounds__(BLEND_T)
blend_rows_kernel(const double *rows, size_t row_stride, size_t samples, const int *__restrict__ first, const int *__restrict__ channel,
                  const double *__restrict__ weight, double *out, size_t out_stride) {
    const int k0 = first[blockIdx.y], k1 = first[blockIdx.y + 1];
    double *dst = out + (size_t)blockIdx.y * out_stride;
    const size_t at = ((size_t)blockIdx.x * BLEND_T + threadIdx.x) * (VEC ? 2 : 1);
    if (at >= samples) return;
    if (VEC && at + 1 < samples) blend_terms<v2d>(rows, row_stride, at, channel, weight, k0, k1, dst);
    else blend_terms<double>(rows, row_stride, at, channel, weight, k0, k1, dst);
}

/* d_out: [n_blends][out_stride]; row r at d_rows + r * row_stride.  The term table lies in device memory: d_first[n_blends + 1],
 * d_channel and d_weight [d_first[n_blends]], checked by the caller (blend.h: every channel a row of d_rows, 1 to 32 terms a blend). */
hipError_t gdg_launch_blend_rows(const double *d_rows, size_t row_stride, size_t samples, unsigned n_blends, const int *d_first, const int *d_channel,
                                 const double *d_weight, double *d_out, size_t out_stride, hipStream_t s) {
    if (n_blends == 0 || samples == 0) return hipSuccess;
    if (!d_rows || !d_out || !d_first || !d_channel || !d_weight || row_stride < samples || out_stride < samples || n_blends > 65535u ||
        ((uintptr_t)d_rows & 7) || ((uintptr_t)d_out & 7) || ((uintptr_t)d_weight & 7) || ((uintptr_t)d_first & 3) || ((uintptr_t)d_channel & 3))
        return hipErrorInvalidValue;
    const bool vec = !((uintptr_t)d_rows & 15) && !(row_stride & 1) && !((uintptr_t)d_out & 15) && !(out_stride & 1);
    const size_t lanes = vec ? (samples + 1) / 2 : samples, tiles = (lanes + BLEND_T - 1) / BLEND_T;
    if (tiles > 0x7fffffffu) return hipErrorInvalidValue;
    const dim3 grid((unsigned)tiles, n_blends);
    if (vec) blend_rows_kernel<true><<<grid, BLEND_T, 0, s>>>(d_rows, row_stride, samples, d_first, d_channel, d_weight, d_out, out_stride);
    else blend_rows_kernel<false><<<grid, BLEND_T, 0, s>>>(d_rows, row_stride, samples, d_first, d_channel, d_weight, d_out, out_stride);
    return hipGetLastError();
}
