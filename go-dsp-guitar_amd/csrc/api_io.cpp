/*
 * api_io.cpp -- either side of the path: wave sample codecs, resample.Time, level meters, power-amp compilation, metronome.
 * Part of the host side of libgdg.so (the C-ABI of include/gdg.h on top of the HIP kernels; see ctx.h for the map).
 * There is no CPU compute path here: every sample is produced by a HIP kernel.
 */
#include "ctx.h"

int ensure_io(gdg_ctx *ctx, int which, size_t bytes) {
    if (ctx->io_cap[which] >= bytes) return GDG_OK;
    if (ctx->d_io[which]) { hipStreamSynchronize(ctx->stream); hipFree(ctx->d_io[which]); ctx->d_io[which] = nullptr; ctx->io_cap[which] = 0; }
    size_t cap = bytes + bytes / 4 + 4096;
    if (hipMalloc(&ctx->d_io[which], cap) != hipSuccess) return fail(ctx, GDG_ERR_NOMEM, "cannot allocate %zu bytes of io scratch", cap);
    ctx->io_cap[which] = cap;
    return GDG_OK;
}

int gdg_wave_bytes_per_sample(int format) {
    static const int w[GDG_FMT_COUNT] = { 1, 2, 3, 4, 4, 8 };
    return (format >= 0 && format < GDG_FMT_COUNT) ? w[format] : 0;
}

int gdg_wave_decode_device(gdg_ctx *ctx, int format, const void *d_bytes, size_t per, unsigned channels, double *d_samples) {
    if (!ctx) return GDG_ERR_INVALID;
    if (!gdg_wave_bytes_per_sample(format)) return fail(ctx, GDG_ERR_UNSUPPORTED, "unknown sample format %d", format);
    if (channels == 0) return fail(ctx, GDG_ERR_INVALID, "channel count must be positive");
    if (per == 0) return GDG_OK;
    if (!d_bytes || !d_samples) return GDG_ERR_INVALID;
    enter_keep_fir_sums(ctx);
    ProfScope ps(ctx, GDG_K_WAVE);
    HIP_TRY(ctx, gdg_launch_wave_decode(format, d_bytes, per, channels, d_samples, ctx->stream));
    return GDG_OK;
}

int gdg_wave_encode_device(gdg_ctx *ctx, int format, const double *d_samples, size_t per, unsigned channels, void *d_bytes) {
    if (!ctx) return GDG_ERR_INVALID;
    if (!gdg_wave_bytes_per_sample(format)) return fail(ctx, GDG_ERR_UNSUPPORTED, "unknown sample format %d", format);
    if (channels == 0) return fail(ctx, GDG_ERR_INVALID, "channel count must be positive");
    if (per == 0) return GDG_OK;
    if (!d_bytes || !d_samples) return GDG_ERR_INVALID;
    enter_keep_fir_sums(ctx);
    ProfScope ps(ctx, GDG_K_WAVE);
    HIP_TRY(ctx, gdg_launch_wave_encode(format, d_samples, per, channels, d_bytes, gdg_encode_mode{}, ctx->stream));
    return GDG_OK;
}

int gdg_wave_decode(gdg_ctx *ctx, int format, const void *bytes, size_t per, unsigned channels, double *samples) {
    if (!ctx) return GDG_ERR_INVALID;
    int w = gdg_wave_bytes_per_sample(format);
    if (!w) return fail(ctx, GDG_ERR_UNSUPPORTED, "unknown sample format %d", format);
    if (channels == 0) return fail(ctx, GDG_ERR_INVALID, "channel count must be positive");
    size_t n = per * channels;
    if (n == 0) return GDG_OK;
    if (!bytes || !samples) return GDG_ERR_INVALID;
    enter_keep_fir_sums(ctx);
    int rc = ensure_io(ctx, 0, n * w);
    if (rc == GDG_OK) rc = ensure_io(ctx, 1, n * sizeof(double));
    if (rc != GDG_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_io[0], bytes, n * w, hipMemcpyHostToDevice, ctx->stream));
    rc = gdg_wave_decode_device(ctx, format, ctx->d_io[0], per, channels, static_cast<double *>(ctx->d_io[1]));
    if (rc != GDG_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(samples, ctx->d_io[1], n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GDG_OK;
}

/* the host form of the three encoders: n samples up, `device_form` from one io buffer into the other, n * width bytes down, synchronised */
template <class F>
static int encode_host(gdg_ctx *ctx, int format, const double *samples, size_t n, void *bytes, F device_form) {
    const size_t w = (size_t)gdg_wave_bytes_per_sample(format);
    enter_keep_fir_sums(ctx);
    int rc = ensure_io(ctx, 0, n * w);
    if (rc == GDG_OK) rc = ensure_io(ctx, 1, n * sizeof(double));
    if (rc != GDG_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_io[1], samples, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    rc = device_form(static_cast<const double *>(ctx->d_io[1]), ctx->d_io[0]);
    if (rc != GDG_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(bytes, ctx->d_io[0], n * w, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GDG_OK;
}

int gdg_wave_encode(gdg_ctx *ctx, int format, const double *samples, size_t per, unsigned channels, void *bytes) {
    if (!ctx) return GDG_ERR_INVALID;
    if (!gdg_wave_bytes_per_sample(format)) return fail(ctx, GDG_ERR_UNSUPPORTED, "unknown sample format %d", format);
    if (channels == 0) return fail(ctx, GDG_ERR_INVALID, "channel count must be positive");
    size_t n = per * channels;
    if (n == 0) return GDG_OK;
    if (!bytes || !samples) return GDG_ERR_INVALID;
    return encode_host(ctx, format, samples, n, bytes, [&](const double *d, void *b) { return gdg_wave_encode_device(ctx, format, d, per, channels, b); });
}

/* the dithered encoder on its own (dither.h): mono; mode 0 and the IEEE formats are gdg_wave_encode's calls, kernels and bytes */
int gdg_wave_encode_dither_device(gdg_ctx *ctx, int format, const double *d_samples, size_t n, int mode, uint64_t seed, uint32_t port, uint64_t first_index,
                                  void *d_bytes) {
    if (!ctx) return GDG_ERR_INVALID;
    if (!gdg_wave_bytes_per_sample(format)) return fail(ctx, GDG_ERR_UNSUPPORTED, "unknown sample format %d", format);
    if (mode != 0 && mode != 1) return fail(ctx, GDG_ERR_INVALID, "encode dither: mode %d; 0 is off, 1 is TPDF", mode);
    if (!gdg_dither_applies(mode, format)) return gdg_wave_encode_device(ctx, format, d_samples, n, 1, d_bytes);
    if (n == 0) return GDG_OK;
    if (!d_bytes || !d_samples) return GDG_ERR_INVALID;
    if ((uintptr_t)d_samples & 7) return fail(ctx, GDG_ERR_INVALID, "encode dither: the samples are float64, 8-byte aligned");
    enter_keep_fir_sums(ctx);
    ProfScope ps(ctx, GDG_K_WAVE);
    const gdg_encode_mode m = { false, true, nullptr, { 1.0, 1.0 }, { seed, first_index, port, 0 } };
    HIP_TRY(ctx, gdg_launch_wave_encode(format, d_samples, n, 1, d_bytes, m, ctx->stream));
    return GDG_OK;
}

int gdg_wave_encode_dither(gdg_ctx *ctx, int format, const double *samples, size_t n, int mode, uint64_t seed, uint32_t port, uint64_t first_index, void *bytes) {
    if (!ctx) return GDG_ERR_INVALID;
    if (!gdg_wave_bytes_per_sample(format)) return fail(ctx, GDG_ERR_UNSUPPORTED, "unknown sample format %d", format);
    if (mode != 0 && mode != 1) return fail(ctx, GDG_ERR_INVALID, "encode dither: mode %d; 0 is off, 1 is TPDF", mode);
    if (!gdg_dither_applies(mode, format)) return gdg_wave_encode(ctx, format, samples, n, 1, bytes);
    if (n == 0) return GDG_OK;
    if (!bytes || !samples) return GDG_ERR_INVALID;
    return encode_host(ctx, format, samples, n, bytes,
                       [&](const double *d, void *b) { return gdg_wave_encode_dither_device(ctx, format, d, n, mode, seed, port, first_index, b); });
}

/* the trimmed encoder on its own (trim.h): mono, y = x * gain in front of gdg_wave_encode_dither's encoder; gain 1.0 is that call itself */
static int encode_trim_check(gdg_ctx *ctx, int format, int mode, double gain) {
    if (!gdg_wave_bytes_per_sample(format)) return fail(ctx, GDG_ERR_UNSUPPORTED, "unknown sample format %d", format);
    if (mode != 0 && mode != 1) return fail(ctx, GDG_ERR_INVALID, "encode trim: mode %d; 0 is the plain encoder, 1 is TPDF dither", mode);
    if (!isfinite(gain)) return fail(ctx, GDG_ERR_INVALID, "encode trim: gain = %g is not finite", gain);
    return GDG_OK;
}

int gdg_wave_encode_trim_device(gdg_ctx *ctx, int format, const double *d_samples, size_t n, double gain, int mode, uint64_t seed, uint32_t port,
                                uint64_t first_index, void *d_bytes) {
    if (!ctx) return GDG_ERR_INVALID;
    const int rc = encode_trim_check(ctx, format, mode, gain);
    if (rc != GDG_OK) return rc;
    if (gain == 1.0) return gdg_wave_encode_dither_device(ctx, format, d_samples, n, mode, seed, port, first_index, d_bytes);
    if (n == 0) return GDG_OK;
    if (!d_bytes || !d_samples) return GDG_ERR_INVALID;
    if ((uintptr_t)d_samples & 7) return fail(ctx, GDG_ERR_INVALID, "encode trim: the samples are float64, 8-byte aligned");
    enter_keep_fir_sums(ctx);
    ProfScope ps(ctx, GDG_K_WAVE);
    const gdg_encode_mode m = { true, gdg_dither_applies(mode, format), nullptr, { gain, gain }, { seed, first_index, port, 0 } };
    HIP_TRY(ctx, gdg_launch_wave_encode(format, d_samples, n, 1, d_bytes, m, ctx->stream));
    return GDG_OK;
}

int gdg_wave_encode_trim(gdg_ctx *ctx, int format, const double *samples, size_t n, double gain, int mode, uint64_t seed, uint32_t port, uint64_t first_index,
                         void *bytes) {
    if (!ctx) return GDG_ERR_INVALID;
    int rc = encode_trim_check(ctx, format, mode, gain);
    if (rc != GDG_OK) return rc;
    if (gain == 1.0) return gdg_wave_encode_dither(ctx, format, samples, n, mode, seed, port, first_index, bytes);
    if (n == 0) return GDG_OK;
    if (!bytes || !samples) return GDG_ERR_INVALID;
    return encode_host(ctx, format, samples, n, bytes,
                       [&](const double *d, void *b) { return gdg_wave_encode_trim_device(ctx, format, d, n, gain, mode, seed, port, first_index, b); });
}

/* the delivery on its own (deliver.h; io.hip, deliver_kernels.h): rows at the session rate -> rows at a half or a quarter of it; factor 1 copies */
static int deliver_check(gdg_ctx *ctx, const char *what, int n_rows, size_t samples, int factor) {
    if (!gdg_deliver_factor_ok(factor)) return fail(ctx, GDG_ERR_INVALID, "%s: delivery factor %d; 1 is the session rate, 2 a half of it, 4 a quarter", what, factor);
    if (n_rows <= 0) return fail(ctx, GDG_ERR_INVALID, "%s: %d rows", what, n_rows);
    if (samples == 0 || samples % (size_t)factor) return fail(ctx, GDG_ERR_INVALID, "%s: %zu samples; a positive multiple of the delivery factor %d", what, samples, factor);
    return GDG_OK;
}

int gdg_deliver_rows_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, int factor, double *d_history, double *d_out,
                            size_t out_stride) {
    if (!ctx) return GDG_ERR_INVALID;
    const int rc = deliver_check(ctx, "deliver rows", n_rows, samples, factor);
    if (rc != GDG_OK) return rc;
    if (!d_rows || !d_out) return GDG_ERR_INVALID;
    if (row_stride < samples || out_stride < samples / (size_t)factor)
        return fail(ctx, GDG_ERR_INVALID, "deliver rows: strides of %zu and %zu samples for rows of %zu and %zu", row_stride, out_stride, samples, samples / (size_t)factor);
    if (((uintptr_t)d_rows & 7) || ((uintptr_t)d_out & 7) || ((uintptr_t)d_history & 7)) return fail(ctx, GDG_ERR_INVALID, "deliver rows: the samples are float64, 8-byte aligned");
    enter_keep_fir_sums(ctx);
    ProfScope ps(ctx, GDG_K_WAVE);
    if (factor == 1)
        HIP_TRY(ctx, hipMemcpy2DAsync(d_out, out_stride * sizeof(double), d_rows, row_stride * sizeof(double), samples * sizeof(double), (size_t)n_rows, hipMemcpyDeviceToDevice, ctx->stream));
    else
        HIP_TRY(ctx, gdg_launch_deliver_rows(factor, d_rows, row_stride, samples, (unsigned)n_rows, factor == 2 ? ctx->os.taps2 : ctx->os.taps4, d_history, d_out, out_stride, ctx->stream));
    /* behind the sum: the rows' last 154 samples are what the next call finds in front of its own */
    if (d_history) HIP_TRY(ctx, gdg_launch_deliver_history_save(d_rows, row_stride, samples, (unsigned)n_rows, d_history, ctx->stream));
    return GDG_OK;
}

int gdg_deliver_rows(gdg_ctx *ctx, const double *rows, int n_rows, size_t samples, int factor, double *history, double *out) {
    if (!ctx) return GDG_ERR_INVALID;
    int rc = deliver_check(ctx, "deliver rows", n_rows, samples, factor);
    if (rc != GDG_OK) return rc;
    if (!rows || !out) return GDG_ERR_INVALID;
    enter_keep_fir_sums(ctx);
    const size_t n_out = samples / (size_t)factor, rows_bytes = ((size_t)n_rows * samples * sizeof(double) + 15) & ~(size_t)15;
    const size_t hist_bytes = history ? (size_t)n_rows * GDG_DELIVER_HISTORY * sizeof(double) : 0;
    rc = ensure_io(ctx, 1, rows_bytes + hist_bytes);
    if (rc == GDG_OK) rc = ensure_io(ctx, 0, (size_t)n_rows * n_out * sizeof(double));
    if (rc != GDG_OK) return rc;
    double *d_rows = static_cast<double *>(ctx->d_io[1]), *d_out = static_cast<double *>(ctx->d_io[0]);
    double *d_hist = history ? reinterpret_cast<double *>(static_cast<unsigned char *>(ctx->d_io[1]) + rows_bytes) : nullptr;
    HIP_TRY(ctx, hipMemcpyAsync(d_rows, rows, (size_t)n_rows * samples * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (history) HIP_TRY(ctx, hipMemcpyAsync(d_hist, history, hist_bytes, hipMemcpyHostToDevice, ctx->stream));
    rc = gdg_deliver_rows_device(ctx, d_rows, samples, n_rows, samples, factor, d_hist, d_out, n_out);
    if (rc != GDG_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out, d_out, (size_t)n_rows * n_out * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (history) HIP_TRY(ctx, hipMemcpyAsync(history, d_hist, hist_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GDG_OK;
}

/* the factor's expanded anti-aliasing taps (aa_taps.h), as the oversampler's table has them: 77 or 155 doubles; pure host arithmetic */
int gdg_deliver_taps(int factor, double *taps, int capacity) {
    const int T = gdg_deliver_tap_count(factor);
    if (!T) return 0;
    const double *half = factor == 2 ? GDG_AA2_HALF : GDG_AA4_HALF;
    for (int k = 0; taps && k < T && k < capacity; k++) taps[k] = half[k <= T / 2 ? k : T - 1 - k];
    return T;
}

/* the ratio stage's prototype (include/gdg.h, DELIVERY): a Kaiser-windowed sinc of L T taps, beta 10, cut off at the Nyquist frequency of the
 * lower rate, gain L; float64 on the host.  I0 by its power series: the terms fall below 1e-17 of the sum within 40 steps at x <= 10. */
static double deliver_i0(double x) {
    double sum = 1.0, term = 1.0;
    const double q = 0.25 * x * x;
    for (int k = 1; k < 200; k++) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}
int deliver_ratio_table(int up, int down, bool transposed, std::vector<double> &taps) {
    const int T = gdg_deliver_ratio_tap_count(up, down), L = up;
    taps.clear();
    if (!T) return 0;
    const double pi = 3.14159265358979323846, beta = 10.0, fc = 0.5 / (double)(up > down ? up : down), c = 0.5 * (double)L * (double)T, i0b = deliver_i0(beta);
    taps.resize((size_t)L * (size_t)T);
    for (int m = 0; m < L * T; m++) {
        const double u = (double)m - c, v = 2.0 * fc * u, r = u / c, inside = 1.0 - r * r;
        const double sinc = v == 0.0 ? 1.0 : sin(pi * v) / (pi * v);
        const double g = (double)L * 2.0 * fc * sinc * deliver_i0(beta * sqrt(inside > 0.0 ? inside : 0.0)) / i0b;
        const int p = m % L, t = m / L;                                        /* tap[p][t] = g[p + t L] */
        taps[transposed ? (size_t)t * (size_t)L + (size_t)p : (size_t)p * (size_t)T + (size_t)t] = g;
    }
    return T;
}

int gdg_out_ratio_taps(int up, int down, double *taps, int capacity) {
    std::vector<double> g;
    if (!deliver_ratio_table(up, down, false, g)) return 0;
    for (size_t k = 0; taps && capacity > 0 && k < g.size() && k < (size_t)capacity; k++) taps[k] = g[k];
    return (int)g.size();
}

size_t gdg_batch_out_samples(int factor, int up, int down, size_t first, size_t count) {
    if (!gdg_deliver_factor_ok(factor) || !gdg_deliver_ratio_ok(up, down) || first % (size_t)factor || count % (size_t)factor) return 0;
    return (size_t)gdg_deliver_samples(factor, up, down, first, count);
}

int gdg_batch_out_ratio_latency(int factor, int up, int down) { return gdg_deliver_ratio_latency(factor, up, down); }

/* what every call refuses of a ratio, in one wording: the reduced pair is named where the caller's is not reduced */
int deliver_ratio_check(gdg_ctx *ctx, const char *what, int up, int down) {
    if (gdg_deliver_ratio_ok(up, down)) return GDG_OK;
    if (up >= 1 && down >= 1) {
        const int g = (int)gdg_deliver_gcd((unsigned long long)up, (unsigned long long)down);
        if (g > 1) return fail(ctx, GDG_ERR_INVALID, "%s: delivery ratio %d/%d is not reduced; pass %d/%d", what, up, down, up / g, down / g);
    }
    return fail(ctx, GDG_ERR_INVALID, "%s: delivery ratio %d/%d; up is 1 to %d, down 1 to %d, down <= 2 up and up <= 2 down", what, up, down, GDG_DELIVER_RATIO_MAX_UP,
                GDG_DELIVER_RATIO_MAX_DOWN);
}

/* the ratio stage on its own (io.hip, deliver_ratio_kernels.h): intermediate rows, the job's [first, first + samples) -> their outputs */
static int deliver_ratio_args(gdg_ctx *ctx, int n_rows, size_t samples, int up, int down, size_t first) {
    const int rc = deliver_ratio_check(ctx, "deliver rows ratio", up, down);
    if (rc != GDG_OK) return rc;
    if (n_rows <= 0) return fail(ctx, GDG_ERR_INVALID, "deliver rows ratio: %d rows at delivery ratio %d/%d", n_rows, up, down);
    if (samples == 0 || samples > ((size_t)1 << 40) || first > ((size_t)1 << 48))
        return fail(ctx, GDG_ERR_INVALID, "deliver rows ratio: %zu samples from %zu on at delivery ratio %d/%d; 1 to 2^40 samples, first up to 2^48", samples, first, up, down);
    return GDG_OK;
}

int gdg_out_ratio_rows_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, int up, int down, size_t first, double *d_history,
                                  double *d_out, size_t out_stride) {
    if (!ctx) return GDG_ERR_INVALID;
    const int rc = deliver_ratio_args(ctx, n_rows, samples, up, down, first);
    if (rc != GDG_OK) return rc;
    if (!d_rows || !d_out) return GDG_ERR_INVALID;
    const size_t n_out = gdg_deliver_ratio_on(up, down) ? (size_t)gdg_deliver_ratio_count(first, samples, up, down) : samples;
    if (row_stride < samples || out_stride < n_out)
        return fail(ctx, GDG_ERR_INVALID, "deliver rows ratio: strides of %zu and %zu samples for rows of %zu and %zu at delivery ratio %d/%d", row_stride, out_stride, samples, n_out, up, down);
    if (((uintptr_t)d_rows & 7) || ((uintptr_t)d_out & 7) || ((uintptr_t)d_history & 7)) return fail(ctx, GDG_ERR_INVALID, "deliver rows ratio: the samples are float64, 8-byte aligned (delivery ratio %d/%d)", up, down);
    enter_keep_fir_sums(ctx);
    ProfScope ps(ctx, GDG_K_WAVE);
    if (!gdg_deliver_ratio_on(up, down)) {
        HIP_TRY(ctx, hipMemcpy2DAsync(d_out, out_stride * sizeof(double), d_rows, row_stride * sizeof(double), samples * sizeof(double), (size_t)n_rows, hipMemcpyDeviceToDevice, ctx->stream));
    } else {
        if (ctx->d_ratio_up != up || ctx->d_ratio_down != down) {             /* another ratio: its table replaces the last one's, behind whatever still reads that */
            std::vector<double> tapsT;
            deliver_ratio_table(up, down, true, tapsT);
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            hipFree(ctx->d_ratio_taps);
            ctx->d_ratio_taps = nullptr;
            ctx->d_ratio_up = ctx->d_ratio_down = 0;
            if (hipMalloc((void **)&ctx->d_ratio_taps, tapsT.size() * sizeof(double)) != hipSuccess)
                return fail(ctx, GDG_ERR_NOMEM, "deliver rows ratio: cannot allocate the %zu taps of delivery ratio %d/%d on the device", tapsT.size(), up, down);
            HIP_TRY(ctx, hipMemcpy(ctx->d_ratio_taps, tapsT.data(), tapsT.size() * sizeof(double), hipMemcpyHostToDevice));
            ctx->d_ratio_up = up;
            ctx->d_ratio_down = down;
        }
        HIP_TRY(ctx, gdg_launch_deliver_ratio(up, down, d_rows, row_stride, samples, (unsigned long long)first, (unsigned)n_rows, ctx->d_ratio_taps, d_history, d_out, out_stride, 0, ctx->stream));
    }
    /* behind the sum: the rows' last 127 samples are what the next call finds in front of its own */
    if (d_history) HIP_TRY(ctx, gdg_launch_deliver_ratio_history_save(d_rows, row_stride, samples, (unsigned)n_rows, d_history, ctx->stream));
    return GDG_OK;
}

int gdg_out_ratio_rows(gdg_ctx *ctx, const double *rows, int n_rows, size_t samples, int up, int down, size_t first, double *history, double *out, size_t out_capacity) {
    if (!ctx) return GDG_ERR_INVALID;
    int rc = deliver_ratio_args(ctx, n_rows, samples, up, down, first);
    if (rc != GDG_OK) return rc;
    if (!rows) return GDG_ERR_INVALID;
    const size_t n_out = gdg_deliver_ratio_on(up, down) ? (size_t)gdg_deliver_ratio_count(first, samples, up, down) : samples;
    if (out_capacity < n_out || (n_out && !out))
        return fail(ctx, GDG_ERR_INVALID, "deliver rows ratio: room for %zu samples per row; %zu samples from %zu on give %zu at delivery ratio %d/%d", out_capacity, samples, first, n_out, up, down);
    enter_keep_fir_sums(ctx);
    const size_t rows_bytes = ((size_t)n_rows * samples * sizeof(double) + 15) & ~(size_t)15;
    const size_t hist_bytes = history ? (size_t)n_rows * GDG_DELIVER_RATIO_HISTORY * sizeof(double) : 0;
    rc = ensure_io(ctx, 1, rows_bytes + hist_bytes);
    if (rc == GDG_OK) rc = ensure_io(ctx, 0, ((size_t)n_rows * n_out + 2) * sizeof(double));
    if (rc != GDG_OK) return rc;
    double *d_rows = static_cast<double *>(ctx->d_io[1]), *d_out = static_cast<double *>(ctx->d_io[0]);
    double *d_hist = history ? reinterpret_cast<double *>(static_cast<unsigned char *>(ctx->d_io[1]) + rows_bytes) : nullptr;
    HIP_TRY(ctx, hipMemcpyAsync(d_rows, rows, (size_t)n_rows * samples * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (history) HIP_TRY(ctx, hipMemcpyAsync(d_hist, history, hist_bytes, hipMemcpyHostToDevice, ctx->stream));
    rc = gdg_out_ratio_rows_device(ctx, d_rows, samples, n_rows, samples, up, down, first, d_hist, d_out, n_out);
    if (rc != GDG_OK) return rc;
    /* the produced outputs only: row r of the caller's buffer begins at out + r * out_capacity */
    if (n_out) HIP_TRY(ctx, hipMemcpy2DAsync(out, out_capacity * sizeof(double), d_out, n_out * sizeof(double), n_out * sizeof(double), (size_t)n_rows, hipMemcpyDeviceToHost, ctx->stream));
    if (history) HIP_TRY(ctx, hipMemcpyAsync(history, d_hist, hist_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GDG_OK;
}

/* the planner (trim.h): pure host arithmetic, no context -- what it refuses is kept per thread for gdg_last_error(NULL) */
/* one planner body for both record kinds: `stride` doubles from one record's true_peak to the next's; `what` words the refusals */
static int trim_from_records(const char *what, const double *true_peaks, size_t stride, bool given, int ports, size_t blocks, double target, double max_gain, double *gain) {
    int bad = -1;
    char msg[160];
    switch (gdg_trim_plan(true_peaks, stride, ports, blocks, target, max_gain, gain, &bad)) {
    case GDG_TRIM_PLAN_OK: return GDG_OK;
    case GDG_TRIM_PLAN_TARGET: snprintf(msg, sizeof msg, "%s: target = %g; finite and greater than 0", what, target); break;
    case GDG_TRIM_PLAN_MAX_GAIN: snprintf(msg, sizeof msg, "%s: max_gain = %g; finite and greater than 0", what, max_gain); break;
    case GDG_TRIM_PLAN_NAN: snprintf(msg, sizeof msg, "%s: port %d has a NaN true_peak", what, bad); break;
    default: snprintf(msg, sizeof msg, "%s: %d ports, records %s, gain %s", what, ports, given ? "given" : "NULL", gain ? "given" : "NULL"); break;
    }
    set_free_error(msg);
    return GDG_ERR_INVALID;
}
int gdg_trim_from_true_peak(const gdg_block_true_peak *records, int ports, size_t blocks, double target, double max_gain, double *gain) {
    static_assert(sizeof(gdg_block_true_peak) == 2 * sizeof(double) && offsetof(gdg_block_true_peak, true_peak) == 0, "the planner strides over true_peak in doubles");
    return trim_from_records("trim from true peak", reinterpret_cast<const double *>(records), 2, records != nullptr, ports, blocks, target, max_gain, gain);
}
/* ... and on the delivered rows' records (include/gdg.h, DELIVERED RECORDS): the same rule on their true_peak, five doubles apart */
int gdg_trim_from_out_records(const gdg_block_delivered *records, int ports, size_t blocks, double target, double max_gain, double *gain) {
    static_assert(sizeof(gdg_block_delivered) == 5 * sizeof(double) && offsetof(gdg_block_delivered, true_peak) == 0, "the planner strides over true_peak in doubles");
    if (ports <= 0 || blocks == 0) {                                          /* no record to plan from: refused, where the true-peak form plans nothing */
        char msg[160];
        snprintf(msg, sizeof msg, "trim from out records: %d ports x %zu blocks; at least one record per port", ports, blocks);
        set_free_error(msg);
        return GDG_ERR_INVALID;
    }
    return trim_from_records("trim from out records", reinterpret_cast<const double *>(records), 5, records != nullptr, ports, blocks, target, max_gain, gain);
}

/* resample/resample.go:72-87 */
int gdg_resample_time_length(int input_length, uint32_t source_rate, uint32_t target_rate) {
    if (input_length < 0 || source_rate == 0 || target_rate == 0) return -1;
    double expansion = (double)target_rate / (double)source_rate;
    double out_len_f = (double)input_length * expansion;
    double out_len_floor = floor(out_len_f);
    int out_len = (int)out_len_floor;
    if (out_len_floor == out_len_f) out_len--;
    return out_len < 0 ? 0 : out_len;
}

int gdg_resample_time_device(gdg_ctx *ctx, const double *d_samples, int n, uint32_t source_rate, uint32_t target_rate, double *d_out, int n_out) {
    if (!ctx) return GDG_ERR_INVALID;
    if (source_rate == 0 || target_rate == 0 || n < 0) return fail(ctx, GDG_ERR_INVALID, "invalid rates or length");
    if (n_out != gdg_resample_time_length(n, source_rate, target_rate))
        return fail(ctx, GDG_ERR_INVALID, "output length %d does not follow the reference's length rule (%d)", n_out,
                    gdg_resample_time_length(n, source_rate, target_rate));
    if (n_out == 0) return GDG_OK;
    if (!d_samples || !d_out) return GDG_ERR_INVALID;
    enter_keep_fir_sums(ctx);
    double dx = (double)source_rate / (double)target_rate;       /* resample.go:88-90 */
    ProfScope ps(ctx, GDG_K_RESAMPLE);
    HIP_TRY(ctx, gdg_launch_resample_time(d_samples, n, dx, d_out, n_out, ctx->stream));
    return GDG_OK;
}

int gdg_resample_time(gdg_ctx *ctx, const double *samples, int n, uint32_t source_rate, uint32_t target_rate, double *out, int n_out) {
    if (!ctx) return GDG_ERR_INVALID;
    if (n_out == 0 && n >= 0 && source_rate && target_rate && gdg_resample_time_length(n, source_rate, target_rate) == 0) return GDG_OK;
    if (!samples || !out || n <= 0 || n_out < 0) return fail(ctx, GDG_ERR_INVALID, "invalid buffers");
    enter_keep_fir_sums(ctx);
    int rc = ensure_io(ctx, 0, (size_t)n * sizeof(double));
    if (rc == GDG_OK) rc = ensure_io(ctx, 1, (size_t)(n_out > 0 ? n_out : 1) * sizeof(double));
    if (rc != GDG_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_io[0], samples, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    rc = gdg_resample_time_device(ctx, static_cast<const double *>(ctx->d_io[0]), n, source_rate, target_rate, static_cast<double *>(ctx->d_io[1]), n_out);
    if (rc != GDG_OK) return rc;
    if (n_out > 0) HIP_TRY(ctx, hipMemcpyAsync(out, ctx->d_io[1], (size_t)n_out * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GDG_OK;
}

/* ---- level meters ----------------------------------------------------------------------------------------- */
#define METER_PEAK_HOLD_SECONDS 2       /* level/level.go:12 */
#define METER_TIME_CONSTANT 1.7         /* level/level.go:13 */
#define METER_MIN_LEVEL (-200.0)        /* level/level.go:14 */

int gdg_meter_configure(gdg_ctx *ctx, int n_ports) {
    if (!ctx || n_ports < 0) return GDG_ERR_INVALID;
    enter_keep_fir_sums(ctx);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->d_meter) { hipFree(ctx->d_meter); ctx->d_meter = nullptr; }
    ctx->n_meter = 0;
    if (n_ports == 0) return GDG_OK;
    if (hipMalloc(&ctx->d_meter, (size_t)n_ports * sizeof(gdg_meter_rec)) != hipSuccess) return fail(ctx, GDG_ERR_NOMEM, "cannot allocate meter state");
    HIP_TRY(ctx, hipMemset(ctx->d_meter, 0, (size_t)n_ports * sizeof(gdg_meter_rec)));
    ctx->n_meter = n_ports;
    return GDG_OK;
}

int gdg_meter_set_enabled(gdg_ctx *ctx, int port, int enabled) {
    if (!ctx) return GDG_ERR_INVALID;
    if (port >= ctx->n_meter) return fail(ctx, GDG_ERR_INVALID, "meter port %d out of range (%d configured)", port, ctx->n_meter);
    if (ctx->n_meter == 0) return GDG_OK;
    enter_keep_fir_sums(ctx);
    std::vector<gdg_meter_rec> st(ctx->n_meter);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(st.data(), ctx->d_meter, st.size() * sizeof(gdg_meter_rec), hipMemcpyDeviceToHost));
    int lo = port < 0 ? 0 : port, hi = port < 0 ? ctx->n_meter : port + 1;
    for (int p = lo; p < hi; p++) {
        if ((enabled != 0) == (st[p].enabled != 0)) continue;           /* level.go:264: only a change acts */
        if (!enabled) { st[p].current = 0.0; st[p].peak = 0.0; st[p].counter = 0; }
        st[p].enabled = enabled != 0;
    }
    HIP_TRY(ctx, hipMemcpy(ctx->d_meter, st.data(), st.size() * sizeof(gdg_meter_rec), hipMemcpyHostToDevice));
    return GDG_OK;
}

/* ports [port0, port0 + n_ports) over one buffer each (rows of d_rows) */
int meter_rows(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int port0, int n_ports, int frames, uint32_t sample_rate) {
    double sr = (double)sample_rate;                                   /* level.go:166-171 */
    unsigned long long hold = (unsigned long long)(METER_PEAK_HOLD_SECONDS * sr);
    double decay = pow(10.0, -1.0 / (METER_TIME_CONSTANT * sr));
    int seg = GDG_METER_SEG;
    if ((unsigned long long)seg > hold) seg = (int)hold;             /* the kernel's single-record argument needs n <= hold */
    ProfScope ps(ctx, GDG_K_METER);
    for (int off = 0; off < frames; off += seg) {
        int n = frames - off < seg ? frames - off : seg;
        HIP_TRY(ctx, gdg_launch_meter(d_rows + off, row_stride, n_ports, n, ctx->d_meter + port0, decay, hold, ctx->stream));
    }
    return GDG_OK;
}

int gdg_meter_process_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int frames, uint32_t sample_rate) {
    if (!ctx) return GDG_ERR_INVALID;
    if (ctx->n_meter == 0 || frames == 0) return GDG_OK;
    if (!d_rows || frames < 0 || sample_rate == 0) return fail(ctx, GDG_ERR_INVALID, "invalid meter input");
    enter_keep_fir_sums(ctx);
    return meter_rows(ctx, d_rows, row_stride, 0, ctx->n_meter, frames, sample_rate);
}

int gdg_meter_process(gdg_ctx *ctx, const double *const *buffers, int frames, uint32_t sample_rate) {
    if (!ctx) return GDG_ERR_INVALID;
    if (ctx->n_meter == 0 || frames == 0) return GDG_OK;
    if (!buffers || frames < 0) return GDG_ERR_INVALID;
    enter_keep_fir_sums(ctx);
    int rc = ensure_io(ctx, 1, (size_t)ctx->n_meter * frames * sizeof(double));
    if (rc != GDG_OK) return rc;
    double *d = static_cast<double *>(ctx->d_io[1]);
    for (int p = 0; p < ctx->n_meter; p++) {
        if (!buffers[p]) return fail(ctx, GDG_ERR_INVALID, "meter buffer %d is null", p);
        HIP_TRY(ctx, hipMemcpyAsync(d + (size_t)p * frames, buffers[p], (size_t)frames * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    rc = gdg_meter_process_device(ctx, d, (size_t)frames, frames, sample_rate);
    if (rc != GDG_OK) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GDG_OK;
}

static int32_t to_decibels_int(double value) {                         /* level.go:100-118 */
    double level = 20.0 * log10(value);
    if (std::isnan(level) || level < METER_MIN_LEVEL) level = METER_MIN_LEVEL;
    return (int32_t)round(level);
}

int gdg_meter_analyze(gdg_ctx *ctx, int32_t *levels, int32_t *peaks) {
    if (!ctx || !levels || !peaks) return GDG_ERR_INVALID;
    if (ctx->n_meter == 0) return GDG_OK;
    enter_keep_fir_sums(ctx);
    std::vector<gdg_meter_rec> st(ctx->n_meter);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(st.data(), ctx->d_meter, st.size() * sizeof(gdg_meter_rec), hipMemcpyDeviceToHost));
    for (int p = 0; p < ctx->n_meter; p++) { levels[p] = to_decibels_int(st[p].current); peaks[p] = to_decibels_int(st[p].peak); }
    return GDG_OK;
}

int gdg_meter_state(gdg_ctx *ctx, int port, double *current, double *peak, uint64_t *counter) {
    if (!ctx || port < 0 || port >= ctx->n_meter) return GDG_ERR_INVALID;
    enter_keep_fir_sums(ctx);
    gdg_meter_rec st;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(&st, ctx->d_meter + port, sizeof(st), hipMemcpyDeviceToHost));
    if (current) *current = st.current;
    if (peak) *peak = st.peak;
    if (counter) *counter = st.counter;
    return GDG_OK;
}

/* ---- power-amp filter compilation on the device (effects/poweramp.go:25-127) ----------------------------------------------- */

int gdg_unit_compile_fir(gdg_ctx *ctx, int handle, int n_filters, const double *const *taps, const int *lengths, const double *gain_compensation,
                         const int32_t *levels_db, uint32_t target_order) {
    Unit *u = get_unit(ctx, handle);
    if (!u) return fail(ctx, GDG_ERR_INVALID, "bad unit handle %d", handle);
    if (u->type != GDG_UNIT_POWERAMP) return fail(ctx, GDG_ERR_INVALID, "unit %d is not a power amp", handle);
    if (n_filters < 0 || (n_filters > 0 && (!taps || !lengths || !gain_compensation || !levels_db))) return fail(ctx, GDG_ERR_INVALID, "bad filter list");
    enter(ctx);
    /* lengths after Reduce, composite length = the longest (filter.go:167-236 Add pads with zeros) */
    size_t max_in = 0, max_out = 0, work_points = 0, pos_points = 0;
    for (int i = 0; i < n_filters; i++) {
        if (!taps[i] || lengths[i] <= 0) continue;                  /* "- NONE -" slot (poweramp.go:78) */
        size_t n = (size_t)lengths[i];
        size_t out = (target_order > 0 && n > (size_t)target_order) ? (size_t)target_order : n;
        if (out != n) {
            size_t w, p;
            gdg_filter_reduce_sizes(lengths[i], target_order, &w, &p);
            if (w > work_points) work_points = w;
            if (p > pos_points) pos_points = p;
        }
        if (n > max_in) max_in = n;
        if (out > max_out) max_out = out;
    }
    std::vector<double> composite(max_out, 0.0);
    if (max_out > 0) {
        /* temporaries from the context's arena (seven hipMalloc / hipFree pairs were 0.7 of a compile's 1.6 ms); every slot has its own
         * upload buffer, so the slots' uploads and kernels queue up behind one another without a host-side wait per slot */
        double *d_in[2] = { nullptr, nullptr }, *d_red = nullptr, *d_comp = nullptr, *d_partial = nullptr;
        double2 *d_wa = nullptr, *d_wb = nullptr, *d_wp = nullptr;
        auto take = [&](void **p, size_t bytes) { return ctx->arena.alloc(p, bytes) == hipSuccess; };
        bool ok = take((void **)&d_in[0], max_in * sizeof(double)) && take((void **)&d_in[1], max_in * sizeof(double));
        ok = ok && take((void **)&d_red, max_out * sizeof(double));
        ok = ok && take((void **)&d_comp, max_out * sizeof(double));
        ok = ok && take((void **)&d_partial, 257 * sizeof(double));
        if (work_points) {
            ok = ok && take((void **)&d_wa, work_points * sizeof(double2));
            ok = ok && take((void **)&d_wb, work_points * sizeof(double2));
            ok = ok && take((void **)&d_wp, pos_points * sizeof(double2));
        }
        hipError_t e = ok ? hipMemsetAsync(d_comp, 0, max_out * sizeof(double), ctx->stream) : hipErrorOutOfMemory;
        int slot = 0;
        for (int i = 0; e == hipSuccess && i < n_filters; i++) {
            if (!taps[i] || lengths[i] <= 0) continue;
            const int n = lengths[i];
            double *d_up = d_in[slot++ & 1];
            /* pageable source: the call returns when the taps have left the caller's buffer; the copy itself is ordered on the stream
             * behind the kernels that read this upload buffer two slots ago */
            e = hipMemcpyAsync(d_up, taps[i], (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
            const double *d_cur = d_up;
            int n_cur = n;
            if (e == hipSuccess && target_order > 0 && (size_t)n > (size_t)target_order) {        /* poweramp.go:88-90 */
                e = gdg_launch_filter_reduce(d_up, n, target_order, d_wa, d_wb, d_wp, d_red, ctx->stream);
                d_cur = d_red;
                n_cur = (int)target_order;
            }
            /* Normalize, Multiply(level), Add (poweramp.go:92-94, :108-118) */
            if (e == hipSuccess)
                e = gdg_launch_normalize_scale_add(d_cur, n_cur, gain_compensation[i], decibels_to_factor(levels_db[i]), d_partial, d_comp, ctx->stream);
        }
        if (e == hipSuccess) e = hipMemcpyAsync(composite.data(), d_comp, max_out * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
        hipError_t e_sync = hipStreamSynchronize(ctx->stream);       /* everything above has run: the temporaries can go back */
        if (e == hipSuccess) e = e_sync;
        ctx->arena.release(d_in[0]); ctx->arena.release(d_in[1]); ctx->arena.release(d_red); ctx->arena.release(d_comp); ctx->arena.release(d_partial);
        ctx->arena.release(d_wa); ctx->arena.release(d_wb); ctx->arena.release(d_wp);
        if (e != hipSuccess) return fail(ctx, e == hipErrorOutOfMemory ? GDG_ERR_NOMEM : GDG_ERR_HIP, "filter compilation failed: %s", hipGetErrorString(e));
    }
    return gdg_unit_set_fir(ctx, handle, composite.data(), (int)composite.size());
}

int gdg_unit_get_fir(gdg_ctx *ctx, int handle, double *taps, int capacity, int *n_taps) {
    Unit *u = get_unit(ctx, handle);
    if (!u) return fail(ctx, GDG_ERR_INVALID, "bad unit handle %d", handle);
    if (u->type != GDG_UNIT_POWERAMP) return fail(ctx, GDG_ERR_INVALID, "unit %d is not a power amp", handle);
    if (n_taps) *n_taps = (int)u->taps.size();
    if (taps) {
        if (capacity < (int)u->taps.size()) return fail(ctx, GDG_ERR_INVALID, "buffer too small for %zu taps", u->taps.size());
        if (!u->taps.empty()) memcpy(taps, u->taps.data(), u->taps.size() * sizeof(double));
    }
    return GDG_OK;
}

/* ---- metronome (metronome/metronome.go) ------------------------------------------------------------------------------------ */

static int set_sound(gdg_ctx *ctx, double **d_buf, uint32_t *n_buf, const double *coeffs, int n) {
    if (n < 0) return fail(ctx, GDG_ERR_INVALID, "bad sound length");
    enter_keep_fir_sums(ctx);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (*d_buf) { hipFree(*d_buf); *d_buf = nullptr; }
    *n_buf = 0;
    if (!coeffs) return GDG_OK;                                    /* SetTick(name, nil): no sound */
    /* a non-nil empty slice is an allocated sound of length 0: keep a one-element allocation so the pointer stays non-null */
    if (hipMalloc((void **)d_buf, (size_t)(n > 0 ? n : 1) * sizeof(double)) != hipSuccess) return fail(ctx, GDG_ERR_NOMEM, "cannot allocate the metronome sound");
    if (n > 0) HIP_TRY(ctx, hipMemcpy(*d_buf, coeffs, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    *n_buf = (uint32_t)n;
    return GDG_OK;
}

int gdg_metronome_set_tick(gdg_ctx *ctx, const double *coefficients, int n) {
    if (!ctx) return GDG_ERR_INVALID;
    return set_sound(ctx, &ctx->d_tick, &ctx->n_tick, coefficients, n);
}

int gdg_metronome_set_tock(gdg_ctx *ctx, const double *coefficients, int n) {
    if (!ctx) return GDG_ERR_INVALID;
    return set_sound(ctx, &ctx->d_tock, &ctx->n_tock, coefficients, n);
}

int gdg_metronome_configure(gdg_ctx *ctx, uint32_t beats_per_period, uint32_t bpm_speed, uint32_t sample_rate) {
    if (!ctx) return GDG_ERR_INVALID;
    if (bpm_speed == 0) return fail(ctx, GDG_ERR_INVALID, "metronome speed must be positive");     /* the reference would divide by zero */
    ctx->met_beats = beats_per_period;
    ctx->met_bpm = bpm_speed;
    ctx->met_sr = sample_rate;
    return GDG_OK;
}

int gdg_metronome_process_device(gdg_ctx *ctx, double *d_out, int frames) {
    if (!ctx || (frames > 0 && !d_out) || frames < 0) return GDG_ERR_INVALID;
    if (frames == 0) return GDG_OK;
    enter_keep_fir_sums(ctx);
    const uint32_t sc0 = ctx->met_sample_counter, tc0 = ctx->met_tick_counter;
    const uint32_t spb = (60u * ctx->met_sr) / ctx->met_bpm;                    /* metronome.go:79, uint32 arithmetic */
    const uint32_t beats = ctx->met_beats == 0 ? 1u : ctx->met_beats;           /* :84-86 */
    /* sample j0 is the first whose increment reaches samples_per_beat (:122-125) */
    const uint32_t j0 = (sc0 + 1u >= spb) ? 0u : (spb - 1u - sc0);
    HIP_TRY(ctx, gdg_launch_metronome(ctx->d_tick, ctx->n_tick, ctx->d_tock, ctx->n_tock, d_out, frames, sc0, tc0, spb, beats, j0, ctx->stream));
    /* counters after the buffer */
    const uint32_t n = (uint32_t)frames;
    if (n - 1u < j0) { ctx->met_sample_counter = sc0 + n; }
    else {
        uint32_t m = n - j0 - 1u;                                               /* samples after the first reset */
        uint32_t resets = 1u + (spb ? m / spb : m);
        ctx->met_sample_counter = spb ? m % spb : 0u;
        ctx->met_tick_counter = ((tc0 + 1u) % beats + (resets - 1u) % beats) % beats;
    }
    return GDG_OK;
}

int gdg_metronome_process(gdg_ctx *ctx, double *out, int frames) {
    if (!ctx || (frames > 0 && !out) || frames < 0) return GDG_ERR_INVALID;
    if (frames == 0) return GDG_OK;
    enter_keep_fir_sums(ctx);
    int rc = ensure_io(ctx, 1, (size_t)frames * sizeof(double));
    if (rc != GDG_OK) return rc;
    rc = gdg_metronome_process_device(ctx, static_cast<double *>(ctx->d_io[1]), frames);
    if (rc != GDG_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out, ctx->d_io[1], (size_t)frames * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GDG_OK;
}

/* ================================================================================================
 * The batch run (controller.processFiles, controller/controller.go:2809-3219, without prompts and file I/O)
 * ============================================================================================== */

/* ---- the render report (include/gdg.h; the kernel: io.hip block_stats_kernel; the batch calls fill it: api_batch.cpp) ------------------ */
static_assert(sizeof(gdg_block_stats) == 32 && offsetof(gdg_block_stats, peak_index) == 16 && offsetof(gdg_block_stats, nonfinite) == 28,
              "gdg_block_stats: 32 bytes, no padding");
static_assert(sizeof(gdg_block_align) == 40, "gdg_block_align: 40 bytes (report_sections.h)");

/* What the four host-pointer entries gdg_block_*_rows share, behind their own checks: the rows go up compact into d_io[1] (an odd `samples`
 * puts every other row 8 bytes past a 16-byte boundary, which the kernels take as it comes), `run` -- the kind's _device entry -- reads
 * them there and writes d_io[0], and `out_bytes` of that come down into `out`; synchronised.  `what` names the kind in a refused row. */
static int rows_round_trip(gdg_ctx *ctx, const char *what, const double *const *rows, int n_rows, size_t samples, void *out, size_t out_bytes,
                           const std::function<int(const double *d_rows, void *d_out)> &run) {
    for (int r = 0; r < n_rows; r++) if (!rows[r]) return fail(ctx, GDG_ERR_INVALID, "%s: row %d is NULL", what, r);
    enter_keep_fir_sums(ctx);
    int rc = ensure_io(ctx, 1, (size_t)n_rows * samples * sizeof(double));
    if (rc == GDG_OK) rc = ensure_io(ctx, 0, out_bytes);
    if (rc != GDG_OK) return rc;
    double *d_rows = static_cast<double *>(ctx->d_io[1]);
    for (int r = 0; r < n_rows; r++)
        HIP_TRY(ctx, hipMemcpyAsync(d_rows + (size_t)r * samples, rows[r], samples * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = run(d_rows, ctx->d_io[0])) != GDG_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out, ctx->d_io[0], out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GDG_OK;
}

/* What the four getters gdg_batch_* share.  The kind's nouns: `none` opens the refusal of a call that kept nothing, `pending` / `without`
 * end it with the switch on / off; `name`, `unit` and `owner` word the refusal of too little room.  Counts out, NULL gives counts alone. */
struct KindWords { const char *none, *pending, *without, *name, *unit, *owner; };
static int batch_kind_get(gdg_ctx *ctx, int kind, bool on, const KindWords &w, void *out, size_t capacity, int *ports, size_t *blocks, int *n_bands) {
    if (!ctx) return GDG_ERR_INVALID;
    const gdg_ctx::ReportKind &K = ctx->report[kind];
    if (!K.valid) return fail(ctx, GDG_ERR_INVALID, "%s: the last batch call of this context %s", w.none, on ? w.pending : w.without);
    const size_t per = kind == REPORT_BANDS ? K.elem / sizeof(double) : 1;      /* values of a port and block: a record, or the bands */
    if (ports) *ports = K.ports;
    if (blocks) *blocks = K.blocks;
    if (n_bands) *n_bands = (int)per;
    if (!out) return GDG_OK;
    const size_t n = (size_t)K.ports * K.blocks * per;
    if (capacity < n) {
        char bands[32] = "";
        if (kind == REPORT_BANDS) snprintf(bands, sizeof bands, " x %zu bands", per);
        return fail(ctx, GDG_ERR_INVALID, "%s: room for %zu %s, the %s has %d ports x %zu blocks%s = %zu", w.name, capacity, w.unit, w.owner, K.ports, K.blocks, bands, n);
    }
    if (n) memcpy(out, K.store.data(), K.store.size());
    return GDG_OK;
}
static int block_stats_check(gdg_ctx *ctx, int n_rows, size_t samples, int block, size_t *blocks) {
    if (n_rows < 0) return fail(ctx, GDG_ERR_INVALID, "block statistics: %d rows", n_rows);
    if (block < 1) return fail(ctx, GDG_ERR_INVALID, "block statistics: blocks of %d samples (at least 1)", block);
    *blocks = (samples + (size_t)block - 1) / (size_t)block;
    if (*blocks > 0x7fffffff) return fail(ctx, GDG_ERR_INVALID, "block statistics: %zu blocks per row are too many for one launch", *blocks);
    return GDG_OK;
}

int gdg_block_stats_rows_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, int block, gdg_block_stats *d_records) {
    if (!ctx) return GDG_ERR_INVALID;
    size_t blocks = 0;
    const int rc = block_stats_check(ctx, n_rows, samples, block, &blocks);
    if (rc != GDG_OK) return rc;
    if (n_rows == 0 || samples == 0) return GDG_OK;
    if (!d_rows || !d_records) return GDG_ERR_INVALID;
    if (row_stride < samples) return fail(ctx, GDG_ERR_INVALID, "block statistics: a row stride of %zu samples for rows of %zu", row_stride, samples);
    if (((uintptr_t)d_rows & 7) || ((uintptr_t)d_records & 7)) return fail(ctx, GDG_ERR_INVALID, "block statistics: rows and records are 8-byte aligned");
    enter_keep_fir_sums(ctx);
    HIP_TRY(ctx, gdg_launch_block_stats(d_rows, row_stride, (unsigned)n_rows, samples, (unsigned)block, d_records, ctx->stream));
    return GDG_OK;
}

int gdg_block_stats_rows(gdg_ctx *ctx, const double *const *rows, int n_rows, size_t samples, int block, gdg_block_stats *records) {
    if (!ctx) return GDG_ERR_INVALID;
    size_t blocks = 0;
    int rc = block_stats_check(ctx, n_rows, samples, block, &blocks);
    if (rc != GDG_OK) return rc;
    if (n_rows == 0 || samples == 0) return GDG_OK;
    if (!rows || !records) return GDG_ERR_INVALID;
    return rows_round_trip(ctx, "block statistics", rows, n_rows, samples, records, (size_t)n_rows * blocks * sizeof(gdg_block_stats), [&](const double *d_rows, void *d_out) {
        return gdg_block_stats_rows_device(ctx, d_rows, samples, n_rows, samples, block, static_cast<gdg_block_stats *>(d_out));
    });
}

int gdg_batch_report_enable(gdg_ctx *ctx, int enable) {
    if (!ctx) return GDG_ERR_INVALID;
    ctx->report_on = enable != 0;              /* read when a batch call begins; the report of the last call stays what it is */
    return GDG_OK;
}

int gdg_batch_report(gdg_ctx *ctx, gdg_block_stats *records, size_t capacity, int *ports, size_t *blocks) {
    static const KindWords words = { "no report", "has not completed (or none has run since gdg_batch_report_enable)",
                                     "ran without one (gdg_batch_report_enable comes before the call)", "report", "records", "report" };
    return batch_kind_get(ctx, REPORT_STATS, ctx && ctx->report_on, words, records, capacity, ports, blocks, nullptr);
}

/* ---- the band spectrum (include/gdg.h; the kernel: spectrum_kernels.h in fir.hip; the edges and bins: spectrum_bands.h; the batch calls fill it: api_batch.cpp) ---- */
int spectrum_tables(gdg_ctx *ctx, const double **win, double2 **tw, double2 **tw2) {
    if (!ctx->d_spec_win) {
        std::vector<double> w((size_t)GDG_SPECTRUM_BLOCK);
        spectrum_window(w.data());
        double *d = nullptr;
        HIP_TRY(ctx, hipMalloc((void **)&d, w.size() * sizeof(double)));
        const hipError_t e = hipMemcpy(d, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice);
        if (e != hipSuccess) { hipFree(d); HIP_TRY(ctx, e); }
        ctx->d_spec_win = d;
    }
    *win = ctx->d_spec_win;
    return fir_tables(ctx, GDG_SPECTRUM_BLOCK / 2, tw, tw2);
}

static int spectrum_edges_refuse(gdg_ctx *ctx, const char *what, const double *edges_hz, int n_edges) {
    int bad = -1;
    switch (spectrum_edges_check(edges_hz, n_edges, &bad)) {
    case SPECTRUM_OK: return GDG_OK;
    case SPECTRUM_COUNT: return fail(ctx, GDG_ERR_INVALID, "%s: %d edges; 2 to %d make 1 to %d bands", what, n_edges, GDG_SPECTRUM_MAX_EDGES, GDG_SPECTRUM_MAX_EDGES - 1);
    case SPECTRUM_NULL: return fail(ctx, GDG_ERR_INVALID, "%s: no edge list", what);
    case SPECTRUM_VALUE: return fail(ctx, GDG_ERR_INVALID, "%s: edge %d is not a finite frequency >= 0", what, bad);
    default: return fail(ctx, GDG_ERR_INVALID, "%s: edge %d does not lie above edge %d (strictly ascending)", what, bad, bad - 1);
    }
}

static int block_spectrum_check(gdg_ctx *ctx, int n_rows, size_t samples, uint32_t sample_rate, const double *edges_hz, int n_edges, size_t *blocks) {
    if (n_rows < 0) return fail(ctx, GDG_ERR_INVALID, "block spectrum: %d rows", n_rows);
    if (sample_rate == 0) return fail(ctx, GDG_ERR_INVALID, "block spectrum: sample rate must be positive");
    const int rc = spectrum_edges_refuse(ctx, "block spectrum", edges_hz, n_edges);
    if (rc != GDG_OK) return rc;
    *blocks = (samples + GDG_SPECTRUM_BLOCK - 1) / GDG_SPECTRUM_BLOCK;
    if (*blocks > 0x7fffffff) return fail(ctx, GDG_ERR_INVALID, "block spectrum: %zu blocks per row are too many for one launch", *blocks);
    return GDG_OK;
}

int gdg_block_spectrum_rows_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, uint32_t sample_rate,
                                   const double *edges_hz, int n_edges, double *d_bands) {
    if (!ctx) return GDG_ERR_INVALID;
    size_t blocks = 0;
    int rc = block_spectrum_check(ctx, n_rows, samples, sample_rate, edges_hz, n_edges, &blocks);
    if (rc != GDG_OK) return rc;
    if (n_rows == 0 || samples == 0) return GDG_OK;
    if (!d_rows || !d_bands) return GDG_ERR_INVALID;
    if (row_stride < samples) return fail(ctx, GDG_ERR_INVALID, "block spectrum: a row stride of %zu samples for rows of %zu", row_stride, samples);
    if (((uintptr_t)d_rows & 7) || ((uintptr_t)d_bands & 7)) return fail(ctx, GDG_ERR_INVALID, "block spectrum: rows and bands are 8-byte aligned");
    enter_keep_fir_sums(ctx);
    const double *win = nullptr;
    double2 *tw = nullptr, *tw2 = nullptr;
    if ((rc = spectrum_tables(ctx, &win, &tw, &tw2)) != GDG_OK) return rc;
    HIP_TRY(ctx, gdg_launch_block_spectrum(d_rows, row_stride, (unsigned)n_rows, samples, win, tw, tw2, spectrum_bands(edges_hz, n_edges, sample_rate), d_bands, ctx->stream));
    return GDG_OK;
}

int gdg_block_spectrum_rows(gdg_ctx *ctx, const double *const *rows, int n_rows, size_t samples, uint32_t sample_rate, const double *edges_hz, int n_edges,
                            double *bands) {
    if (!ctx) return GDG_ERR_INVALID;
    size_t blocks = 0;
    int rc = block_spectrum_check(ctx, n_rows, samples, sample_rate, edges_hz, n_edges, &blocks);
    if (rc != GDG_OK) return rc;
    if (n_rows == 0 || samples == 0) return GDG_OK;
    if (!rows || !bands) return GDG_ERR_INVALID;
    return rows_round_trip(ctx, "block spectrum", rows, n_rows, samples, bands, (size_t)n_rows * blocks * (size_t)(n_edges - 1) * sizeof(double), [&](const double *d_rows, void *d_out) {
        return gdg_block_spectrum_rows_device(ctx, d_rows, samples, n_rows, samples, sample_rate, edges_hz, n_edges, static_cast<double *>(d_out));
    });
}

int gdg_batch_spectrum_enable(gdg_ctx *ctx, const double *edges_hz, int n_edges) {
    if (!ctx) return GDG_ERR_INVALID;
    if (ctx->bstream.open)
        return fail(ctx, GDG_ERR_INVALID, "batch spectrum: a streamed batch run is open on this context; its setting holds until gdg_batch_stream_close");
    if (n_edges == 0) { ctx->spec_edges.clear(); return GDG_OK; }             /* off; the spectrum of the last call stays what it is */
    int rc = spectrum_edges_refuse(ctx, "batch spectrum", edges_hz, n_edges);   /* the whole list, before it replaces the one in force */
    if (rc != GDG_OK) return rc;
    const double *win = nullptr;
    double2 *tw = nullptr, *tw2 = nullptr;
    enter(ctx, true);                                                        /* configuration: no state of the context changes */
    if ((rc = spectrum_tables(ctx, &win, &tw, &tw2)) != GDG_OK) return rc;     /* made here: no batch call allocates or uploads them */
    ctx->spec_edges.assign(edges_hz, edges_hz + n_edges);
    return GDG_OK;
}

int gdg_batch_spectrum(gdg_ctx *ctx, double *bands, size_t capacity, int *ports, size_t *blocks, int *n_bands) {
    static const KindWords words = { "no spectrum", "has not completed (or none has run since gdg_batch_spectrum_enable)",
                                     "ran without one (gdg_batch_spectrum_enable comes before the call)", "spectrum", "values", "spectrum" };
    return batch_kind_get(ctx, REPORT_BANDS, ctx && !ctx->spec_edges.empty(), words, bands, capacity, ports, blocks, n_bands);
}

/* ---- the alignment report (include/gdg.h; the kernel: align_kernels.h in fir.hip; the list's validation: align_map.h; the batch calls fill it: api_batch.cpp) ---- */
static int align_refuse(gdg_ctx *ctx, const char *what, int status, int n_ports, int max_lag, int bad, const int *ref) {
    switch (status) {
    case ALIGN_OK: return GDG_OK;
    case ALIGN_COUNT: return fail(ctx, GDG_ERR_INVALID, "%s: a list of %d ports", what, n_ports);
    case ALIGN_NULL: return fail(ctx, GDG_ERR_INVALID, "%s: no reference list", what);
    case ALIGN_LAG: return fail(ctx, GDG_ERR_INVALID, "%s: a lag range of %d; 1 to %d", what, max_lag, GDG_ALIGN_MAX_LAG);
    default: return fail(ctx, GDG_ERR_INVALID, "%s: port %d names reference %d; -1 or a port below %d", what, bad, ref[bad], n_ports);
    }
}

static int block_align_check(gdg_ctx *ctx, int n_rows, size_t samples, const int *ref, int max_lag, size_t *blocks) {
    if (n_rows < 0) return fail(ctx, GDG_ERR_INVALID, "block align: %d rows", n_rows);
    if (n_rows > 0) {
        int bad = -1;
        const int st = align_map_check(ref, n_rows, max_lag, &bad);
        if (st != ALIGN_OK) return align_refuse(ctx, "block align", st, n_rows, max_lag, bad, ref);
    } else if (max_lag < 1 || max_lag > GDG_ALIGN_MAX_LAG) return align_refuse(ctx, "block align", ALIGN_LAG, n_rows, max_lag, -1, ref);
    *blocks = (samples + GDG_ALIGN_BLOCK - 1) / GDG_ALIGN_BLOCK;
    if (*blocks > 0x7fffffff) return fail(ctx, GDG_ERR_INVALID, "block align: %zu blocks per row are too many for one launch", *blocks);
    return GDG_OK;
}

int gdg_block_align_rows_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, const int *ref, int max_lag,
                                gdg_block_align *d_records) {
    if (!ctx) return GDG_ERR_INVALID;
    size_t blocks = 0;
    int rc = block_align_check(ctx, n_rows, samples, ref, max_lag, &blocks);
    if (rc != GDG_OK) return rc;
    if (n_rows == 0 || samples == 0) return GDG_OK;
    if (!d_rows || !d_records) return GDG_ERR_INVALID;
    if (row_stride < samples) return fail(ctx, GDG_ERR_INVALID, "block align: a row stride of %zu samples for rows of %zu", row_stride, samples);
    if (((uintptr_t)d_rows & 7) || ((uintptr_t)d_records & 7)) return fail(ctx, GDG_ERR_INVALID, "block align: rows and records are 8-byte aligned");
    enter_keep_fir_sums(ctx);
    double2 *tw = nullptr, *tw2 = nullptr;
    if ((rc = fir_tables(ctx, GDG_ALIGN_BLOCK, &tw, &tw2)) != GDG_OK) return rc;
    HIP_TRY(ctx, hipMemsetAsync(d_records, 0, (size_t)n_rows * blocks * sizeof(gdg_block_align), ctx->stream));      /* an unmeasured row: zeros */
    for (const gdg_align_pairs &q : align_map_pieces(std::vector<int>(ref, ref + n_rows), max_lag))
        HIP_TRY(ctx, gdg_launch_block_align(d_rows, row_stride, (unsigned)n_rows, 0u, (unsigned)n_rows, samples, q, tw, d_records, ctx->stream));
    return GDG_OK;
}

int gdg_block_align_rows(gdg_ctx *ctx, const double *const *rows, int n_rows, size_t samples, const int *ref, int max_lag, gdg_block_align *records) {
    if (!ctx) return GDG_ERR_INVALID;
    size_t blocks = 0;
    int rc = block_align_check(ctx, n_rows, samples, ref, max_lag, &blocks);
    if (rc != GDG_OK) return rc;
    if (n_rows == 0 || samples == 0) return GDG_OK;
    if (!rows || !records) return GDG_ERR_INVALID;
    return rows_round_trip(ctx, "block align", rows, n_rows, samples, records, (size_t)n_rows * blocks * sizeof(gdg_block_align), [&](const double *d_rows, void *d_out) {
        return gdg_block_align_rows_device(ctx, d_rows, samples, n_rows, samples, ref, max_lag, static_cast<gdg_block_align *>(d_out));
    });
}

int gdg_batch_align_enable(gdg_ctx *ctx, const int *ref, int n_ports, int max_lag) {
    if (!ctx) return GDG_ERR_INVALID;
    if (ctx->bstream.open)
        return fail(ctx, GDG_ERR_INVALID, "batch align: a streamed batch run is open on this context; its setting holds until gdg_batch_stream_close");
    if (!ref || n_ports == 0) { ctx->align_ref.clear(); ctx->align_lag = 0; return GDG_OK; }      /* off; the records of the last call stay what they are */
    int bad = -1;
    const int st = align_map_check(ref, n_ports, max_lag, &bad);                /* the whole list, before it replaces the one in force */
    if (st != ALIGN_OK) return align_refuse(ctx, "batch align", st, n_ports, max_lag, bad, ref);
    double2 *tw = nullptr, *tw2 = nullptr;
    enter(ctx, true);                                                        /* configuration: no state of the context changes */
    const int rc = fir_tables(ctx, GDG_ALIGN_BLOCK, &tw, &tw2);                /* made here: no batch call allocates or uploads them */
    if (rc != GDG_OK) return rc;
    align_map_replace(ctx->align_ref, ctx->align_lag, ref, n_ports, max_lag, &bad);
    return GDG_OK;
}

int gdg_batch_align(gdg_ctx *ctx, gdg_block_align *records, size_t capacity, int *ports, size_t *blocks) {
    static const KindWords words = { "no alignment records", "has not completed, was a master finish, or none has run since gdg_batch_align_enable",
                                     "ran without them (gdg_batch_align_enable comes before the call)", "alignment", "records", "call" };
    return batch_kind_get(ctx, REPORT_ALIGN, ctx && !ctx->align_ref.empty(), words, records, capacity, ports, blocks, nullptr);
}

/* ---- the blend on its own (include/gdg.h; the kernels and their launcher: blend_kernels.h in io.hip; the list, its table and its view: blend.h; the batch calls:
 * api_batch.cpp).  The plain, the delayed and the filtered call are one device body and one host body; a form passes null for what it lacks ---- */
static int blend_rows_check(gdg_ctx *ctx, int n_rows, int n_blends, const int *first, const int *channel, const double *weight, const int *delay, const int *tap_first,
                            const double *tap) {
    if (n_rows < 1) return fail(ctx, GDG_ERR_INVALID, "blend rows: %d rows (at least 1)", n_rows);
    int b = -1, k = -1, t = -1;
    char msg[240];
    if (const int rc = gdg_blend_check(n_blends, first, channel, weight, delay, nullptr, n_rows, &b, &k)) {
        gdg_blend_list_message(msg, sizeof msg, "blend rows", true, rc, b, k, n_blends, first, channel, weight, delay, nullptr, n_rows);
        return fail(ctx, GDG_ERR_INVALID, "%s", msg);
    }
    if (const int rc = gdg_blend_check_taps(n_blends, first, delay, tap_first, tap, &b, &k, &t)) {
        gdg_blend_taps_message(msg, sizeof msg, "blend rows", rc, b, k, t, first, delay, tap_first, tap, n_blends);
        return fail(ctx, GDG_ERR_INVALID, "%s", msg);
    }
    return GDG_OK;
}

/* The table is the caller's host memory: it is taken as the batch takes a list in force (gdg_blend_replace: delays that are all 0 and taps
 * that are none are dropped, so such a list runs the kernel of the form without them), goes up, the kernel runs, and the call returns when
 * the rows are written.  The history is held against its rules whether or not the kernel will read it. */
static int blend_rows_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, int n_blends, const int *first, const int *channel,
                             const double *weight, const int *delay, const int *tap_first, const double *tap, const double *d_history, size_t hist_stride, double *d_out,
                             size_t out_stride) {
    if (!ctx) return GDG_ERR_INVALID;
    const int rc = blend_rows_check(ctx, n_rows, n_blends, first, channel, weight, delay, tap_first, tap);
    if (rc != GDG_OK) return rc;
    if (n_blends == 0 || samples == 0) return GDG_OK;
    if (!d_rows || !d_out) return GDG_ERR_INVALID;
    if (row_stride < samples || out_stride < samples) return fail(ctx, GDG_ERR_INVALID, "blend rows: strides of %zu and %zu samples for rows of %zu", row_stride, out_stride, samples);
    if (((uintptr_t)d_rows & 7) || ((uintptr_t)d_out & 7)) return fail(ctx, GDG_ERR_INVALID, "blend rows: rows and sums are 8-byte aligned");
    if (d_history && (((uintptr_t)d_history & 7) || hist_stride < (size_t)GDG_BLEND_MAX_DELAY))
        return fail(ctx, GDG_ERR_INVALID, "blend rows: the history is 8-byte aligned, a row's run has %d samples; its stride is %zu", GDG_BLEND_MAX_DELAY, hist_stride);
    enter_keep_fir_sums(ctx);
    BlendSet set;
    int b = -1, k = -1;
    gdg_blend_replace(set, n_blends, first, channel, weight, delay, tap_first, tap, nullptr, n_rows, &b, &k);      /* checked above: it cannot refuse */
    void *d = nullptr;
    HIP_TRY(ctx, ctx->arena.alloc(&d, set.packed.size()));
    hipError_t e = hipMemcpyAsync(d, set.packed.data(), set.packed.size(), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        ProfScope ps(ctx, GDG_K_WAVE);
        e = gdg_launch_blend(set.view(d), d_rows, row_stride, samples, d_history, hist_stride, d_out, out_stride, ctx->stream);
    }
    const hipError_t w = hipStreamSynchronize(ctx->stream);
    ctx->arena.release(d);
    if (e != hipSuccess) return fail(ctx, GDG_ERR_HIP, "blend rows: %s", hipGetErrorString(e));
    if (w != hipSuccess) return fail(ctx, GDG_ERR_HIP, "blend rows: %s", hipGetErrorString(w));
    return GDG_OK;
}

/* rows, history (null: none) and sums in host memory: the history goes up, the rows make the round trip through the device body */
static int blend_rows_host(gdg_ctx *ctx, const double *const *rows, int n_rows, size_t samples, int n_blends, const int *first, const int *channel, const double *weight,
                           const int *delay, const int *tap_first, const double *tap, const double *const *history, double *const *out) {
    if (!ctx) return GDG_ERR_INVALID;
    int rc = blend_rows_check(ctx, n_rows, n_blends, first, channel, weight, delay, tap_first, tap);
    if (rc != GDG_OK) return rc;
    if (n_blends == 0 || samples == 0) return GDG_OK;
    if (!rows || !out) return GDG_ERR_INVALID;
    for (int b = 0; b < n_blends; b++) if (!out[b]) return fail(ctx, GDG_ERR_INVALID, "blend rows: the row of blend %d is NULL", b);
    if (history) for (int r = 0; r < n_rows; r++) if (!history[r]) return fail(ctx, GDG_ERR_INVALID, "blend rows: the history of row %d is NULL", r);
    const size_t H = (size_t)GDG_BLEND_MAX_DELAY;
    void *d_hist = nullptr;
    if (history) {
        enter_keep_fir_sums(ctx);
        HIP_TRY(ctx, ctx->arena.alloc(&d_hist, (size_t)n_rows * H * sizeof(double)));
        for (int r = 0; r < n_rows; r++) {
            const hipError_t e = hipMemcpyAsync(static_cast<double *>(d_hist) + (size_t)r * H, history[r], H * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
            if (e != hipSuccess) {
                hipStreamSynchronize(ctx->stream);
                ctx->arena.release(d_hist);
                return fail(ctx, GDG_ERR_HIP, "blend rows: %s", hipGetErrorString(e));
            }
        }
    }
    std::vector<double> sums((size_t)n_blends * samples);
    rc = rows_round_trip(ctx, "blend rows", rows, n_rows, samples, sums.data(), sums.size() * sizeof(double), [&](const double *d_rows, void *d_out) {
        return blend_rows_device(ctx, d_rows, samples, n_rows, samples, n_blends, first, channel, weight, delay, tap_first, tap, static_cast<const double *>(d_hist), H,
                                 static_cast<double *>(d_out), samples);
    });
    if (d_hist) {
        hipStreamSynchronize(ctx->stream);
        ctx->arena.release(d_hist);
    }
    if (rc != GDG_OK) return rc;
    for (int b = 0; b < n_blends; b++) memcpy(out[b], sums.data() + (size_t)b * samples, samples * sizeof(double));
    return GDG_OK;
}

int gdg_blend_rows_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, int n_blends, const int *first, const int *channel,
                          const double *weight, double *d_out, size_t out_stride) {
    return blend_rows_device(ctx, d_rows, row_stride, n_rows, samples, n_blends, first, channel, weight, nullptr, nullptr, nullptr, nullptr, 0, d_out, out_stride);
}

int gdg_blend_rows(gdg_ctx *ctx, const double *const *rows, int n_rows, size_t samples, int n_blends, const int *first, const int *channel, const double *weight,
                   double *const *out) {
    return blend_rows_host(ctx, rows, n_rows, samples, n_blends, first, channel, weight, nullptr, nullptr, nullptr, nullptr, out);
}

int gdg_blend_rows_delayed_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, int n_blends, const int *first,
                                  const int *channel, const double *weight, const int *delay, const double *d_history, size_t hist_stride, double *d_out,
                                  size_t out_stride) {
    return blend_rows_device(ctx, d_rows, row_stride, n_rows, samples, n_blends, first, channel, weight, delay, nullptr, nullptr, d_history, hist_stride, d_out, out_stride);
}

int gdg_blend_rows_delayed(gdg_ctx *ctx, const double *const *rows, int n_rows, size_t samples, int n_blends, const int *first, const int *channel,
                           const double *weight, const int *delay, const double *const *history, double *const *out) {
    return blend_rows_host(ctx, rows, n_rows, samples, n_blends, first, channel, weight, delay, nullptr, nullptr, history, out);
}

int gdg_blend_rows_filtered_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, int n_blends, const int *first,
                                   const int *channel, const double *weight, const int *delay, const int *tap_first, const double *tap, const double *d_history,
                                   size_t hist_stride, double *d_out, size_t out_stride) {
    return blend_rows_device(ctx, d_rows, row_stride, n_rows, samples, n_blends, first, channel, weight, delay, tap_first, tap, d_history, hist_stride, d_out, out_stride);
}

int gdg_blend_rows_filtered(gdg_ctx *ctx, const double *const *rows, int n_rows, size_t samples, int n_blends, const int *first, const int *channel,
                            const double *weight, const int *delay, const int *tap_first, const double *tap, const double *const *history, double *const *out) {
    return blend_rows_host(ctx, rows, n_rows, samples, n_blends, first, channel, weight, delay, tap_first, tap, history, out);
}

/* the taps of a fractional delay (blend.h): pure host arithmetic, no context */
int gdg_blend_fraction_taps(int n_taps, double fraction, double *tap) {
    if (gdg_blend_fraction_taps_plan(n_taps, fraction, tap)) return GDG_OK;
    char msg[200];
    snprintf(msg, sizeof msg, "blend fraction taps: %d taps (even, 2 to %d) for a fraction of %g (0 <= fraction < 1); tap is needed", n_taps, GDG_BLEND_MAX_TAPS, fraction);
    set_free_error(msg);
    return GDG_ERR_INVALID;
}

/* the planner (blend.h): pure host arithmetic, no context -- what it refuses is kept per thread for gdg_last_error(NULL) */
int gdg_blend_delays_from_align(const gdg_block_align *records, int ports, size_t blocks, const int *ref, double min_coeff, int n_blends, const int *first,
                                const int *channel, int *delay, int *sign) {
    static_assert(sizeof(gdg_blend_align_rec) == sizeof(gdg_block_align) && offsetof(gdg_blend_align_rec, corr) == offsetof(gdg_block_align, corr) &&
                  offsetof(gdg_blend_align_rec, ref_sq) == offsetof(gdg_block_align, ref_sq) && offsetof(gdg_blend_align_rec, sq_at_lag) == offsetof(gdg_block_align, sq_at_lag) &&
                  offsetof(gdg_blend_align_rec, lag) == offsetof(gdg_block_align, lag), "blend.h restates gdg_block_align");
    int bad = -1;
    char msg[200];
    switch (gdg_blend_plan_delays(reinterpret_cast<const gdg_blend_align_rec *>(records), ports, blocks, ref, min_coeff, n_blends, first, channel, delay, sign, &bad)) {
    case BLEND_PLAN_OK: return GDG_OK;
    case BLEND_PLAN_LIST: snprintf(msg, sizeof msg, "blend delays from align: blend %d: 1 to %d terms, offsets from 0 that ascend, every channel and its reference a port below %d", bad, GDG_BLEND_MAX_TERMS, ports); break;
    case BLEND_PLAN_MIXED: snprintf(msg, sizeof msg, "blend delays from align: blend %d: its terms are not measured against one reference port", bad); break;
    default: snprintf(msg, sizeof msg, "blend delays from align: %d ports, %d blends, min_coeff = %g (0 to 1); records, ref, first, channel, delay and sign are needed", ports, n_blends, min_coeff); break;
    }
    set_free_error(msg);
    return GDG_ERR_INVALID;
}

/* ---- the blend fit (include/gdg.h, FIT; the kernel: fit_kernels.h in io.hip; the list's validation and the planner: blend.h; the batch calls fill it: api_batch.cpp) ---- */
static_assert(sizeof(gdg_block_fit) == FIT_RECORD_BYTES && offsetof(gdg_block_fit, tx) == 8 && offsetof(gdg_block_fit, xx) == 72 && offsetof(gdg_block_fit, skipped) == 360 &&
              offsetof(gdg_block_fit, terms) == 364, "gdg_block_fit: 368 bytes, no padding (report_sections.h)");
static_assert(sizeof(gdg_blend_fit_rec) == sizeof(gdg_block_fit) && offsetof(gdg_blend_fit_rec, tx) == offsetof(gdg_block_fit, tx) &&
              offsetof(gdg_blend_fit_rec, xx) == offsetof(gdg_block_fit, xx) && offsetof(gdg_blend_fit_rec, terms) == offsetof(gdg_block_fit, terms), "blend.h restates gdg_block_fit");

/* A list of fits held against gdg_fit_check, refused in the words of the call `what`: the ONE place they are worded.  n_rows >= 0: the ports
 * name rows 0 .. n_rows - 1 (the stand-alone forms); n_rows < 0: ports of a job to come, whose count is checked when it is described. */
int fit_list_check(gdg_ctx *ctx, const char *what, int n_fits, const int *first, const int *port, const int *target, int n_rows) {
    int f = -1, k = -1;
    switch (gdg_fit_check(n_fits, first, port, target, n_rows, &f, &k)) {
    case FIT_OK: return GDG_OK;
    case FIT_COUNT: return fail(ctx, GDG_ERR_INVALID, "%s: %d fits; 0 (off) to %d", what, n_fits, GDG_FIT_MAX_FITS);
    case FIT_NULL: return fail(ctx, GDG_ERR_INVALID, "%s: %d fits need first, port and target", what, n_fits);
    case FIT_FIRST: return fail(ctx, GDG_ERR_INVALID, "%s: fit %d: first[%d] = %d, first[%d] = %d; the offsets start at 0 and never descend", what, f, f, first[f], f + 1, first[f + 1]);
    case FIT_TERMS: return fail(ctx, GDG_ERR_INVALID, "%s: fit %d has %d terms; 1 to %d", what, f, first[f + 1] - first[f], GDG_FIT_MAX_TERMS);
    case FIT_PORT:
        if (n_rows >= 0) return fail(ctx, GDG_ERR_INVALID, "%s: fit %d, term %d names row %d of %d", what, f, k, port[first[f] + k], n_rows);
        return fail(ctx, GDG_ERR_INVALID, "%s: fit %d, term %d names port %d; ports start at 0", what, f, k, port[first[f] + k]);
    default:
        if (n_rows >= 0) return fail(ctx, GDG_ERR_INVALID, "%s: fit %d has the target row %d of %d", what, f, target[f], n_rows);
        return fail(ctx, GDG_ERR_INVALID, "%s: fit %d has the target port %d; ports start at 0", what, f, target[f]);
    }
}

/* What the stand-alone calls and the getters of the three list records share (report_sections.h, LIST_KINDS; their list checks above and
 * below differ and stay).  The rows, block and blocks-limit refusals around a kind's list check, in the words of the call `what`; `one`:
 * "launch" or "call", as the kind words its limit. */
template <class ListCheck>
static int block_list_check(gdg_ctx *ctx, const char *what, const char *one, int n_rows, size_t samples, int block, const ListCheck &list_check, size_t *blocks) {
    if (n_rows < 1) return fail(ctx, GDG_ERR_INVALID, "%s: %d rows (at least 1)", what, n_rows);
    if (block < 1) return fail(ctx, GDG_ERR_INVALID, "%s: blocks of %d samples (at least 1)", what, block);
    const int rc = list_check();
    if (rc != GDG_OK) return rc;
    *blocks = (samples + (size_t)block - 1) / (size_t)block;
    if (*blocks > 0x7fffffff) return fail(ctx, GDG_ERR_INVALID, "%s: %zu blocks per row are too many for one %s", what, *blocks, one);
    return GDG_OK;
}

/* The device body of kind k behind its checked list: the table of `ints` ints is host memory -- it goes up, the kernel runs, and the call
 * returns when the records are written */
static int block_list_rows_device(gdg_ctx *ctx, int k, const char *what, const double *d_rows, size_t row_stride, int n_rows, size_t samples, int block, const int *table,
                                  size_t ints, int count, void *d_records) {
    if (!d_rows || !d_records) return GDG_ERR_INVALID;
    if (row_stride < samples) return fail(ctx, GDG_ERR_INVALID, "%s: a row stride of %zu samples for rows of %zu", what, row_stride, samples);
    if (((uintptr_t)d_rows & 7) || ((uintptr_t)d_records & 7)) return fail(ctx, GDG_ERR_INVALID, "%s: rows and records are 8-byte aligned", what);
    enter_keep_fir_sums(ctx);
    void *d = nullptr;
    HIP_TRY(ctx, ctx->arena.alloc(&d, ints * sizeof(int)));
    hipError_t e = hipMemcpyAsync(d, table, ints * sizeof(int), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        ProfScope ps(ctx, GDG_K_WAVE);
        e = list_launch[k](d_rows, row_stride, (unsigned)n_rows, samples, (unsigned)block, table, static_cast<const int *>(d), (unsigned)count, d_records, ctx->stream);
    }
    const hipError_t w = hipStreamSynchronize(ctx->stream);
    ctx->arena.release(d);
    if (e != hipSuccess) return fail(ctx, GDG_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    if (w != hipSuccess) return fail(ctx, GDG_ERR_HIP, "%s: %s", what, hipGetErrorString(w));
    return GDG_OK;
}

/* The getter of kind k: its own store, by the four kinds' rule and in their words (KindWords above): `none` opens the refusal of a call that
 * kept nothing, `pending` / `without` end it with the list in force / off; `name` and `unit` word the refusal of too little room -- capacity
 * counts records for the fits and the delivered rows' records and doubles for the other three.  NULL gives the count of blocks alone. */
struct ListWords { const char *none, *pending, *without, *name, *unit; };
static int batch_list_get(gdg_ctx *ctx, int k, const ListWords &w, void *out, size_t capacity, size_t *blocks) {
    if (!ctx) return GDG_ERR_INVALID;
    const gdg_ctx::ListRecords &R = ctx->list_rec[k];
    /* in force or not does not hang on a call's ports: the shape of no ports answers for every kind */
    if (!R.valid) return fail(ctx, GDG_ERR_INVALID, "%s: the last batch call of this context %s", w.none, list_in_force(ctx, k, 0).shape.on() ? w.pending : w.without);
    if (blocks) *blocks = R.blocks;
    if (!out) return GDG_OK;
    const bool records = k == LIST_FIT || k == LIST_DELIVERED;
    const size_t n = records ? R.rows * R.blocks : R.store.size() / sizeof(double);
    if (capacity < n) {
        char has[64];
        if (k == LIST_FIT) snprintf(has, sizeof has, "%d fits x %zu blocks", R.count, R.blocks);
        else if (k == LIST_DELIVERED) snprintf(has, sizeof has, "%d ports x %zu blocks", R.count, R.blocks);
        else if (k == LIST_GRAM) snprintf(has, sizeof has, "%zu blocks x %d (%d + 1) / 2", R.blocks, R.count, R.count);
        else snprintf(has, sizeof has, "%zu blocks x %zu", R.blocks, R.elem / sizeof(double));
        return fail(ctx, GDG_ERR_INVALID, "%s: room for %zu %s, the call has %s = %zu", w.name, capacity, w.unit, has, n);
    }
    if (n) memcpy(out, R.store.data(), R.store.size());
    return GDG_OK;
}

static int block_fit_check(gdg_ctx *ctx, int n_rows, size_t samples, int block, int n_fits, const int *first, const int *port, const int *target, size_t *blocks) {
    return block_list_check(ctx, "block fit", "launch", n_rows, samples, block, [&] { return fit_list_check(ctx, "block fit", n_fits, first, port, target, n_rows); }, blocks);
}

int gdg_block_fit_rows_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, int block, int n_fits, const int *first,
                              const int *port, const int *target, gdg_block_fit *d_records) {
    if (!ctx) return GDG_ERR_INVALID;
    size_t blocks = 0;
    const int rc = block_fit_check(ctx, n_rows, samples, block, n_fits, first, port, target, &blocks);
    if (rc != GDG_OK) return rc;
    if (n_fits == 0 || samples == 0) return GDG_OK;
    const std::vector<int> table = gdg_fit_table(n_fits, first, port, target);
    return block_list_rows_device(ctx, LIST_FIT, "block fit", d_rows, row_stride, n_rows, samples, block, table.data(), table.size(), n_fits, d_records);
}

int gdg_block_fit_rows(gdg_ctx *ctx, const double *const *rows, int n_rows, size_t samples, int block, int n_fits, const int *first, const int *port,
                       const int *target, gdg_block_fit *records) {
    if (!ctx) return GDG_ERR_INVALID;
    size_t blocks = 0;
    const int rc = block_fit_check(ctx, n_rows, samples, block, n_fits, first, port, target, &blocks);
    if (rc != GDG_OK) return rc;
    if (n_fits == 0 || samples == 0) return GDG_OK;
    if (!rows || !records) return GDG_ERR_INVALID;
    return rows_round_trip(ctx, "block fit", rows, n_rows, samples, records, (size_t)n_fits * blocks * sizeof(gdg_block_fit), [&](const double *d_rows, void *d_out) {
        return gdg_block_fit_rows_device(ctx, d_rows, samples, n_rows, samples, block, n_fits, first, port, target, static_cast<gdg_block_fit *>(d_out));
    });
}

int gdg_batch_fit(gdg_ctx *ctx, gdg_block_fit *records, size_t capacity, int *fits, size_t *blocks) {
    static const ListWords words = { "no fit records", "has not completed, was a master finish, or none has run since gdg_batch_fit_enable",
                                     "ran without them (gdg_batch_fit_enable comes before the call)", "fit", "records" };
    if (ctx && fits && ctx->list_rec[LIST_FIT].valid) *fits = ctx->list_rec[LIST_FIT].count;
    return batch_list_get(ctx, LIST_FIT, words, records, capacity, blocks);
}

/* the planner (blend.h): pure host arithmetic, no context -- what it refuses is kept per thread for gdg_last_error(NULL) */
int gdg_blend_weights_from_fit(const gdg_block_fit *records, int n_fits, size_t blocks, double ridge, double *weight, double *residual) {
    int bad = -1;
    char msg[240];
    switch (gdg_blend_plan_weights(reinterpret_cast<const gdg_blend_fit_rec *>(records), n_fits, blocks, ridge, weight, residual, &bad)) {
    case FIT_PLAN_OK: return GDG_OK;
    case FIT_PLAN_TERMS: snprintf(msg, sizeof msg, "blend weights from fit: fit %d: its records do not agree on a term count in 1 to %d", bad, GDG_FIT_MAX_TERMS); break;
    case FIT_PLAN_PIVOT:
        snprintf(msg, sizeof msg, "blend weights from fit: fit %d: a pivot at or below K * 2^-52 * max(diag G) -- a silent term, or a port used twice with ridge = 0", bad);
        break;
    default: snprintf(msg, sizeof msg, "blend weights from fit: %d fits (0 to %d) of %zu blocks (at least 1), ridge = %g (finite, >= 0); records, weight and residual are needed", n_fits, GDG_FIT_MAX_FITS, blocks, ridge); break;
    }
    set_free_error(msg);
    return GDG_ERR_INVALID;
}

/* the fraction of a delay from fit records (blend.h): pure host arithmetic, no context */
int gdg_blend_fractions_from_fit(const gdg_block_fit *records, int n_fits, size_t blocks, int steps, int *step) {
    int bad = -1;
    char msg[240];
    switch (gdg_blend_plan_fractions(reinterpret_cast<const gdg_blend_fit_rec *>(records), n_fits, blocks, steps, step, &bad)) {
    case FRACTION_OK: return GDG_OK;
    case FRACTION_TERMS: snprintf(msg, sizeof msg, "blend fractions from fit: fit %d: a record has another term count than 2 * %d - 1 = %d candidates", bad, steps, 2 * steps - 1); break;
    case FRACTION_NONFINITE: snprintf(msg, sizeof msg, "blend fractions from fit: fit %d: a sum over its %zu blocks is a NaN or inf", bad, blocks); break;
    default: snprintf(msg, sizeof msg, "blend fractions from fit: %d fits (0 to %d) of %zu blocks (at least 1), steps = %d (1 to 4); records and step are needed", n_fits, GDG_FIT_MAX_FITS, blocks, steps); break;
    }
    set_free_error(msg);
    return GDG_ERR_INVALID;
}

/* ---- the Gram of a port list (include/gdg.h, GRAM; the kernel: gram_kernels.h in gram.hip; the list's checks and the planner: blend.h; the batch calls fill it: api_batch.cpp) ---- */
int gram_list_check(gdg_ctx *ctx, const char *what, const int *port, int n_ports, int least, int n_rows) {
    if (n_ports < least || n_ports > GDG_GRAM_MAX_PORTS) return fail(ctx, GDG_ERR_INVALID, "%s: a list of %d ports; %d to %d", what, n_ports, least, GDG_GRAM_MAX_PORTS);
    if (!port) return fail(ctx, GDG_ERR_INVALID, "%s: %d ports need a list", what, n_ports);
    const int bad = gdg_gram_list_bad(port, n_ports, n_rows);
    if (bad >= 0 && n_rows >= 0) return fail(ctx, GDG_ERR_INVALID, "%s: list entry %d names row %d of %d", what, bad, port[bad], n_rows);
    if (bad >= 0) return fail(ctx, GDG_ERR_INVALID, "%s: list entry %d names port %d; ports start at 0", what, bad, port[bad]);
    int earlier = -1;
    const int again = gdg_gram_list_repeat(port, n_ports, &earlier);
    if (again >= 0) return fail(ctx, GDG_ERR_INVALID, "%s: list entry %d names port %d, which entry %d names already", what, again, port[again], earlier);
    return GDG_OK;
}

static int block_gram_check(gdg_ctx *ctx, int n_rows, size_t samples, int block, const int *port, int n_ports, size_t *blocks) {
    return block_list_check(ctx, "block gram", "call", n_rows, samples, block, [&] { return gram_list_check(ctx, "block gram", port, n_ports, 1, n_rows); }, blocks);
}

int gdg_block_gram_rows_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, int block, const int *port, int n_ports, double *d_records) {
    if (!ctx) return GDG_ERR_INVALID;
    size_t blocks = 0;
    const int rc = block_gram_check(ctx, n_rows, samples, block, port, n_ports, &blocks);
    if (rc != GDG_OK) return rc;
    if (samples == 0) return GDG_OK;
    return block_list_rows_device(ctx, LIST_GRAM, "block gram", d_rows, row_stride, n_rows, samples, block, port, (size_t)n_ports, n_ports, d_records);
}

int gdg_block_gram_rows(gdg_ctx *ctx, const double *const *rows, int n_rows, size_t samples, int block, const int *port, int n_ports, double *records) {
    if (!ctx) return GDG_ERR_INVALID;
    size_t blocks = 0;
    const int rc = block_gram_check(ctx, n_rows, samples, block, port, n_ports, &blocks);
    if (rc != GDG_OK) return rc;
    if (samples == 0) return GDG_OK;
    if (!rows || !records) return GDG_ERR_INVALID;
    return rows_round_trip(ctx, "block gram", rows, n_rows, samples, records, blocks * gram_record_bytes((size_t)n_ports), [&](const double *d_rows, void *d_out) {
        return gdg_block_gram_rows_device(ctx, d_rows, samples, n_rows, samples, block, port, n_ports, static_cast<double *>(d_out));
    });
}

/* capacity in doubles */
int gdg_batch_gram(gdg_ctx *ctx, double *out, size_t capacity, size_t *blocks) {
    static const ListWords words = { "no Gram records", "has not completed, was a master finish, or none has run since gdg_batch_gram_enable",
                                     "ran without them (gdg_batch_gram_enable comes before the call)", "gram", "doubles" };
    return batch_list_get(ctx, LIST_GRAM, words, out, capacity, blocks);
}

/* the planner (blend.h): pure host arithmetic, no context -- what it refuses is kept per thread for gdg_last_error(NULL) */
int gdg_blend_pick_from_gram(const double *records, int n_ports, size_t blocks, int target, const int *candidate, int n_candidates, int max_terms, double ridge,
                             double min_gain, int *picked, double *weight, double *residual, int *n_picked) {
    int at = -1;
    char msg[280];
    switch (gdg_blend_pick(records, n_ports, blocks, target, candidate, n_candidates, max_terms, ridge, min_gain, picked, weight, residual, n_picked, &at)) {
    case PICK_OK: return GDG_OK;
    case PICK_POSITION:
        if (at < 0) snprintf(msg, sizeof msg, "blend pick from gram: the target is list position %d of %d", target, n_ports);
        else snprintf(msg, sizeof msg, "blend pick from gram: candidate %d is list position %d of %d", at, candidate[at], n_ports);
        break;
    case PICK_REPEAT: snprintf(msg, sizeof msg, "blend pick from gram: candidate %d is list position %d, which is the target or an earlier candidate", at, candidate[at]); break;
    case PICK_NONFINITE: snprintf(msg, sizeof msg, "blend pick from gram: the summed Gram has a NaN or inf entry at list position %d (the block statistics count non-finite samples per port)", at); break;
    case PICK_SILENT: snprintf(msg, sizeof msg, "blend pick from gram: the target (list position %d) is silent: its energy over the %zu blocks is not above 0", target, blocks); break;
    default:
        snprintf(msg, sizeof msg, "blend pick from gram: %d ports (2 to %d), %zu blocks (at least 1), %d candidates (1 to ports - 1), max_terms = %d (1 to %d), ridge = %g and "
                 "min_gain = %g (finite, >= 0); records, candidate, picked, weight, residual and n_picked are needed", n_ports, GDG_GRAM_MAX_PORTS, blocks, n_candidates, max_terms,
                 GDG_FIT_MAX_TERMS, ridge, min_gain);
        break;
    }
    set_free_error(msg);
    return GDG_ERR_INVALID;
}

/* ---- the tap fit (include/gdg.h, TAPFIT; the kernel: tapfit_kernels.h in gram.hip; the list's validation and the planner: blend.h; the batch calls fill it: api_batch.cpp) ---- */
/* A list of tap fits held against gdg_tapfit_check, refused in the words of the call `what`: the ONE place they are worded; n_rows as for the fits */
int tapfit_list_check(gdg_ctx *ctx, const char *what, int n_fits, const int *first, const int *port, const int *target, const int *taps, int n_rows) {
    int f = -1, k = -1;
    switch (gdg_tapfit_check(n_fits, first, port, target, taps, n_rows, &f, &k)) {
    case TAPFIT_OK: return GDG_OK;
    case TAPFIT_COUNT: return fail(ctx, GDG_ERR_INVALID, "%s: %d fits; 0 (off) to %d", what, n_fits, GDG_TAPFIT_MAX_FITS);
    case TAPFIT_NULL: return fail(ctx, GDG_ERR_INVALID, "%s: %d fits need first, port, target and taps", what, n_fits);
    case TAPFIT_FIRST: return fail(ctx, GDG_ERR_INVALID, "%s: fit %d: first[%d] = %d, first[%d] = %d; the offsets start at 0 and never descend", what, f, f, first[f], f + 1, first[f + 1]);
    case TAPFIT_TERMS: return fail(ctx, GDG_ERR_INVALID, "%s: fit %d has %d terms; 1 to %d", what, f, first[f + 1] - first[f], GDG_TAPFIT_MAX_TERMS);
    case TAPFIT_TAPS: return fail(ctx, GDG_ERR_INVALID, "%s: fit %d has %d taps per term; 1 to %d", what, f, taps[f], GDG_BLEND_MAX_TAPS);
    case TAPFIT_UNKNOWNS:
        return fail(ctx, GDG_ERR_INVALID, "%s: fit %d has %d terms x %d taps = %d unknowns; at most %d", what, f, first[f + 1] - first[f], taps[f], (first[f + 1] - first[f]) * taps[f],
                    GDG_TAPFIT_MAX_UNKNOWNS);
    case TAPFIT_PORT:
        if (n_rows >= 0) return fail(ctx, GDG_ERR_INVALID, "%s: fit %d, term %d names row %d of %d", what, f, k, port[first[f] + k], n_rows);
        return fail(ctx, GDG_ERR_INVALID, "%s: fit %d, term %d names port %d; ports start at 0", what, f, k, port[first[f] + k]);
    default:
        if (n_rows >= 0) return fail(ctx, GDG_ERR_INVALID, "%s: fit %d has the target row %d of %d", what, f, target[f], n_rows);
        return fail(ctx, GDG_ERR_INVALID, "%s: fit %d has the target port %d; ports start at 0", what, f, target[f]);
    }
}

/* D: pure arithmetic; 0 for a list it cannot size */
size_t gdg_tapfit_doubles(int n_fits, const int *first, const int *taps) {
    if (n_fits < 1 || !first || !taps) return 0;
    for (int f = 0; f < n_fits; f++) if (first[f + 1] < first[f] || taps[f] < 0) return 0;
    return gdg_tapfit_list_doubles(n_fits, first, taps);
}

static int block_tapfit_check(gdg_ctx *ctx, int n_rows, size_t samples, int block, int n_fits, const int *first, const int *port, const int *target, const int *taps, size_t *blocks) {
    return block_list_check(ctx, "block tapfit", "call", n_rows, samples, block,
                            [&] { return tapfit_list_check(ctx, "block tapfit", n_fits, first, port, target, taps, n_rows); }, blocks);
}

int gdg_block_tapfit_rows_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, int block, int n_fits, const int *first,
                                 const int *port, const int *target, const int *taps, double *d_records) {
    if (!ctx) return GDG_ERR_INVALID;
    size_t blocks = 0;
    const int rc = block_tapfit_check(ctx, n_rows, samples, block, n_fits, first, port, target, taps, &blocks);
    if (rc != GDG_OK) return rc;
    if (n_fits == 0 || samples == 0) return GDG_OK;
    const std::vector<int> table = gdg_tapfit_table(n_fits, first, port, target, taps);
    return block_list_rows_device(ctx, LIST_TAPFIT, "block tapfit", d_rows, row_stride, n_rows, samples, block, table.data(), table.size(), n_fits, d_records);
}

int gdg_block_tapfit_rows(gdg_ctx *ctx, const double *const *rows, int n_rows, size_t samples, int block, int n_fits, const int *first, const int *port,
                          const int *target, const int *taps, double *records) {
    if (!ctx) return GDG_ERR_INVALID;
    size_t blocks = 0;
    const int rc = block_tapfit_check(ctx, n_rows, samples, block, n_fits, first, port, target, taps, &blocks);
    if (rc != GDG_OK) return rc;
    if (n_fits == 0 || samples == 0) return GDG_OK;
    if (!rows || !records) return GDG_ERR_INVALID;
    return rows_round_trip(ctx, "block tapfit", rows, n_rows, samples, records, blocks * gdg_tapfit_list_doubles(n_fits, first, taps) * sizeof(double), [&](const double *d_rows, void *d_out) {
        return gdg_block_tapfit_rows_device(ctx, d_rows, samples, n_rows, samples, block, n_fits, first, port, target, taps, static_cast<double *>(d_out));
    });
}

/* capacity in doubles */
int gdg_batch_tapfit(gdg_ctx *ctx, double *out, size_t capacity, size_t *blocks, size_t *doubles_per_block) {
    static const ListWords words = { "no tap-fit records", "has not completed, was a master finish, or none has run since gdg_batch_tapfit_enable",
                                     "ran without them (gdg_batch_tapfit_enable comes before the call)", "tapfit", "doubles" };
    if (ctx && doubles_per_block && ctx->list_rec[LIST_TAPFIT].valid) *doubles_per_block = ctx->list_rec[LIST_TAPFIT].elem / sizeof(double);
    return batch_list_get(ctx, LIST_TAPFIT, words, out, capacity, blocks);
}

/* the planner (blend.h): pure host arithmetic, no context -- what it refuses is kept per thread for gdg_last_error(NULL) */
int gdg_blend_taps_from_tapfit(const double *records, int n_fits, const int *first, const int *taps, size_t blocks, double ridge, double *tap, double *residual) {
    int bad = -1, row = -1;
    char msg[320];
    const int rc = gdg_blend_plan_taps(records, n_fits, first, taps, blocks, ridge, tap, residual, &bad, &row);
    if (rc == TAPS_PLAN_OK) return GDG_OK;
    const int T = (bad >= 0 && taps && taps[bad] > 0) ? taps[bad] : 1, U = (bad >= 0 && first && taps) ? (first[bad + 1] - first[bad]) * taps[bad] : 0;
    switch (rc) {
    case TAPS_PLAN_NONFINITE:
        if (row >= U) snprintf(msg, sizeof msg, "blend taps from tapfit: fit %d: the summed record has a NaN or inf entry in the target's row", bad);
        else snprintf(msg, sizeof msg, "blend taps from tapfit: fit %d, term %d, lag %d: the summed record has a NaN or inf entry in that row", bad, row / T, row % T);
        break;
    case TAPS_PLAN_PIVOT:
        snprintf(msg, sizeof msg, "blend taps from tapfit: fit %d, term %d, lag %d: a pivot at or below U * 2^-52 * max(diag A) -- a silent or band-limited term, or a port used twice; "
                 "try ridge > 0", bad, row / T, row % T);
        break;
    default:
        snprintf(msg, sizeof msg, "blend taps from tapfit: %d fits (0 to %d) of %zu blocks (at least 1), ridge = %g (finite, >= 0), every fit 1 to %d terms x 1 to %d taps, at most %d "
                 "unknowns (fit %d); records, first, taps, tap and residual are needed", n_fits, GDG_TAPFIT_MAX_FITS, blocks, ridge, GDG_TAPFIT_MAX_TERMS, GDG_BLEND_MAX_TAPS,
                 GDG_TAPFIT_MAX_UNKNOWNS, bad);
        break;
    }
    set_free_error(msg);
    return GDG_ERR_INVALID;
}

/* ---- the transfer records (include/gdg.h, TRANSFER; the kernel: transfer_kernels.h in fir.hip; the list's validation and the planner: blend.h; the batch calls fill it: api_batch.cpp) ---- */
/* A transfer list held against gdg_transfer_check, refused in the words of the call `what`: the ONE place they are worded; n_rows as for the fits */
int transfer_list_check(gdg_ctx *ctx, const char *what, int n_pairs, const int *port, const int *target, int group, int n_rows) {
    int q = -1;
    switch (gdg_transfer_check(n_pairs, port, target, group, n_rows, &q)) {
    case TRANSFER_OK: return GDG_OK;
    case TRANSFER_COUNT: return fail(ctx, GDG_ERR_INVALID, "%s: %d pairs; 0 (off) to %d", what, n_pairs, GDG_TRANSFER_MAX_PAIRS);
    case TRANSFER_NULL: return fail(ctx, GDG_ERR_INVALID, "%s: %d pairs need port and target", what, n_pairs);
    case TRANSFER_GROUP: return fail(ctx, GDG_ERR_INVALID, "%s: a group width of %d bins; 1, 2, 4, 8, 16, 32 or %d", what, group, GDG_TRANSFER_MAX_GROUP);
    case TRANSFER_PORT:
        if (n_rows >= 0) return fail(ctx, GDG_ERR_INVALID, "%s: pair %d names row %d of %d", what, q, port[q], n_rows);
        return fail(ctx, GDG_ERR_INVALID, "%s: pair %d names port %d; ports start at 0", what, q, port[q]);
    default:
        if (n_rows >= 0) return fail(ctx, GDG_ERR_INVALID, "%s: pair %d has the target row %d of %d", what, q, target[q], n_rows);
        return fail(ctx, GDG_ERR_INVALID, "%s: pair %d has the target port %d; ports start at 0", what, q, target[q]);
    }
}

/* n_pairs (4096 / D + 1) 4: pure arithmetic; 0 for a list it cannot size */
size_t gdg_transfer_doubles(int n_pairs, int group) { return gdg_transfer_list_doubles(n_pairs, group); }

static int block_transfer_check(gdg_ctx *ctx, int n_rows, size_t samples, int n_pairs, const int *port, const int *target, int group, size_t *blocks) {
    if (n_rows < 1) return fail(ctx, GDG_ERR_INVALID, "block transfer: %d rows (at least 1)", n_rows);
    if (n_pairs < 1) return fail(ctx, GDG_ERR_INVALID, "block transfer: %d pairs; 1 to %d", n_pairs, GDG_TRANSFER_MAX_PAIRS);
    const int rc = transfer_list_check(ctx, "block transfer", n_pairs, port, target, group, n_rows);
    if (rc != GDG_OK) return rc;
    *blocks = (samples + GDG_TRANSFER_BLOCK - 1) / GDG_TRANSFER_BLOCK;
    if (*blocks > 0x7fffffff) return fail(ctx, GDG_ERR_INVALID, "block transfer: %zu blocks per row are too many for one call", *blocks);
    return GDG_OK;
}

/* the table goes up, the kernel runs, and the call returns when the records are written */
int gdg_block_transfer_rows_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, int n_pairs, const int *port, const int *target,
                                   int group, double *d_records) {
    if (!ctx) return GDG_ERR_INVALID;
    size_t blocks = 0;
    int rc = block_transfer_check(ctx, n_rows, samples, n_pairs, port, target, group, &blocks);
    if (rc != GDG_OK) return rc;
    if (samples == 0) return GDG_OK;
    if (!d_rows || !d_records) return GDG_ERR_INVALID;
    if (row_stride < samples) return fail(ctx, GDG_ERR_INVALID, "block transfer: a row stride of %zu samples for rows of %zu", row_stride, samples);
    if (((uintptr_t)d_rows & 7) || ((uintptr_t)d_records & 7)) return fail(ctx, GDG_ERR_INVALID, "block transfer: rows and records are 8-byte aligned");
    enter_keep_fir_sums(ctx);
    double2 *tw = nullptr, *tw2 = nullptr;
    if ((rc = fir_tables(ctx, GDG_TRANSFER_BLOCK, &tw, &tw2)) != GDG_OK) return rc;
    const std::vector<int> table = gdg_transfer_table(n_pairs, port, target, group);
    void *d = nullptr;
    HIP_TRY(ctx, ctx->arena.alloc(&d, table.size() * sizeof(int)));
    hipError_t e = hipMemcpyAsync(d, table.data(), table.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        ProfScope ps(ctx, GDG_K_WAVE);
        e = gdg_launch_block_transfer(d_rows, row_stride, (unsigned)n_rows, samples, table.data(), static_cast<const int *>(d), (unsigned)n_pairs, tw, d_records, ctx->stream);
    }
    const hipError_t w = hipStreamSynchronize(ctx->stream);
    ctx->arena.release(d);
    if (e != hipSuccess) return fail(ctx, GDG_ERR_HIP, "block transfer: %s", hipGetErrorString(e));
    if (w != hipSuccess) return fail(ctx, GDG_ERR_HIP, "block transfer: %s", hipGetErrorString(w));
    return GDG_OK;
}

int gdg_block_transfer_rows(gdg_ctx *ctx, const double *const *rows, int n_rows, size_t samples, int n_pairs, const int *port, const int *target, int group,
                            double *records) {
    if (!ctx) return GDG_ERR_INVALID;
    size_t blocks = 0;
    const int rc = block_transfer_check(ctx, n_rows, samples, n_pairs, port, target, group, &blocks);
    if (rc != GDG_OK) return rc;
    if (samples == 0) return GDG_OK;
    if (!rows || !records) return GDG_ERR_INVALID;
    return rows_round_trip(ctx, "block transfer", rows, n_rows, samples, records, blocks * gdg_transfer_list_doubles(n_pairs, group) * sizeof(double), [&](const double *d_rows, void *d_out) {
        return gdg_block_transfer_rows_device(ctx, d_rows, samples, n_rows, samples, n_pairs, port, target, group, static_cast<double *>(d_out));
    });
}

/* capacity in doubles */
int gdg_batch_transfer(gdg_ctx *ctx, double *out, size_t capacity, size_t *blocks, size_t *doubles_per_block) {
    static const ListWords words = { "no transfer records", "has not completed, was a master finish, or none has run since gdg_batch_transfer_enable",
                                     "ran without them (gdg_batch_transfer_enable comes before the call)", "transfer", "doubles" };
    if (ctx && doubles_per_block && ctx->list_rec[LIST_TRANSFER].valid) *doubles_per_block = ctx->list_rec[LIST_TRANSFER].elem / sizeof(double);
    return batch_list_get(ctx, LIST_TRANSFER, words, out, capacity, blocks);
}

/* the planner (blend.h): pure host arithmetic, no context -- what it refuses is kept per thread for gdg_last_error(NULL) */
int gdg_match_taps_from_transfer(const double *records, int n_pairs, int group, size_t blocks, double ridge, int n_taps, int center, double *tap, double *coherence) {
    int bad = -1;
    char msg[320];
    switch (gdg_match_plan_taps(records, n_pairs, group, blocks, ridge, n_taps, center, tap, coherence, &bad)) {
    case MATCH_PLAN_OK: return GDG_OK;
    case MATCH_PLAN_NONFINITE: snprintf(msg, sizeof msg, "match taps from transfer: pair %d: the summed record has a NaN or inf entry", bad); break;
    case MATCH_PLAN_SILENT: snprintf(msg, sizeof msg, "match taps from transfer: pair %d: the summed record has no energy in the port (every Sxx is 0): nothing to divide by", bad); break;
    default:
        snprintf(msg, sizeof msg, "match taps from transfer: %d pairs (0 to %d) of %zu blocks (at least 1), group = %d (1, 2, 4 .. %d), ridge = %g (finite, >= 0), n_taps = %d (1 to "
                 "N' / 2 = 4096 / group), center = %d (0 to n_taps - 1); records, tap and coherence are needed", n_pairs, GDG_TRANSFER_MAX_PAIRS, blocks, group,
                 GDG_TRANSFER_MAX_GROUP, ridge, n_taps, center);
        break;
    }
    set_free_error(msg);
    return GDG_ERR_INVALID;
}

/* ---- the true-peak record (include/gdg.h; the kernel: true_peak_kernels.h in io.hip; the taps: true_peak_taps.h; the batch calls fill it: api_batch.cpp) ---- */
static_assert(sizeof(gdg_block_true_peak) == 16 && offsetof(gdg_block_true_peak, position) == 8 && offsetof(gdg_block_true_peak, overs) == 12,
              "gdg_block_true_peak: 16 bytes, no padding");
const gdg_true_peak_table &true_peak_table() {
    static const gdg_true_peak_table table = [] { gdg_true_peak_table t; true_peak_build(&t); return t; }();
    return table;
}

int gdg_true_peak_taps(double *taps, int capacity) { return true_peak_copy(&true_peak_table(), taps, capacity) ? GDG_OK : GDG_ERR_INVALID; }

static int block_true_peak_check(gdg_ctx *ctx, int n_rows, size_t samples, size_t *blocks) {
    if (n_rows <= 0) return fail(ctx, GDG_ERR_INVALID, "block true peak: %d rows (at least 1)", n_rows);
    *blocks = (samples + GDG_TRUE_PEAK_BLOCK - 1) / GDG_TRUE_PEAK_BLOCK;
    if (*blocks > 0x7fffffff) return fail(ctx, GDG_ERR_INVALID, "block true peak: %zu blocks per row are too many for one launch", *blocks);
    return GDG_OK;
}

int gdg_block_true_peak_rows_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, gdg_block_true_peak *d_records) {
    if (!ctx) return GDG_ERR_INVALID;
    size_t blocks = 0;
    const int rc = block_true_peak_check(ctx, n_rows, samples, &blocks);
    if (rc != GDG_OK) return rc;
    if (samples == 0) return GDG_OK;
    if (!d_rows || !d_records) return fail(ctx, GDG_ERR_INVALID, "block true peak: %s is NULL", !d_rows ? "the rows' pointer" : "the records' pointer");
    if (row_stride < samples) return fail(ctx, GDG_ERR_INVALID, "block true peak: a row stride of %zu samples for rows of %zu", row_stride, samples);
    if (((uintptr_t)d_rows & 7) || ((uintptr_t)d_records & 7)) return fail(ctx, GDG_ERR_INVALID, "block true peak: rows and records are 8-byte aligned");
    enter_keep_fir_sums(ctx);
    HIP_TRY(ctx, gdg_launch_block_true_peak(d_rows, row_stride, (unsigned)n_rows, samples, true_peak_table(), d_records, ctx->stream));
    return GDG_OK;
}

int gdg_block_true_peak_rows(gdg_ctx *ctx, const double *const *rows, int n_rows, size_t samples, gdg_block_true_peak *records) {
    if (!ctx) return GDG_ERR_INVALID;
    size_t blocks = 0;
    int rc = block_true_peak_check(ctx, n_rows, samples, &blocks);
    if (rc != GDG_OK) return rc;
    if (samples == 0) return GDG_OK;
    if (!rows || !records) return fail(ctx, GDG_ERR_INVALID, "block true peak: %s is NULL", !rows ? "the rows' list" : "the records' pointer");
    return rows_round_trip(ctx, "block true peak", rows, n_rows, samples, records, (size_t)n_rows * blocks * sizeof(gdg_block_true_peak), [&](const double *d_rows, void *d_out) {
        return gdg_block_true_peak_rows_device(ctx, d_rows, samples, n_rows, samples, static_cast<gdg_block_true_peak *>(d_out));
    });
}

int gdg_batch_true_peak_enable(gdg_ctx *ctx, int enable) {
    if (!ctx) return GDG_ERR_INVALID;
    if (ctx->bstream.open)
        return fail(ctx, GDG_ERR_INVALID, "batch true peak: a streamed batch run is open on this context; its setting holds until gdg_batch_stream_close");
    ctx->tp_on = enable != 0;                  /* read when a batch call begins; the records of the last call stay what they are */
    return GDG_OK;
}

int gdg_batch_true_peak(gdg_ctx *ctx, gdg_block_true_peak *records, size_t capacity, int *ports, size_t *blocks) {
    static const KindWords words = { "no true-peak records", "has not completed (or none has run since gdg_batch_true_peak_enable)",
                                     "ran without them (gdg_batch_true_peak_enable comes before the call)", "true peak", "records", "call" };
    return batch_kind_get(ctx, REPORT_TRUE_PEAK, ctx && ctx->tp_on, words, records, capacity, ports, blocks, nullptr);
}

/* ---- the records of the delivered rows (include/gdg.h, DELIVERED RECORDS; the kernels: delivered_kernels.h in io.hip; the batch calls fill them: api_batch.cpp) ---- */
static_assert(sizeof(gdg_block_delivered) == DELIVERED_RECORD_BYTES && offsetof(gdg_block_delivered, true_peak) == 0 && offsetof(gdg_block_delivered, position) == 24 &&
              offsetof(gdg_block_delivered, clipped) == 36, "gdg_block_delivered: 40 bytes, no padding");

/* rows, samples and the spans: ascending from 0 to `samples`, every block 1 to 16384 samples */
static int block_out_check(gdg_ctx *ctx, int n_rows, size_t samples, const size_t *span, size_t n_blocks) {
    if (n_rows <= 0) return fail(ctx, GDG_ERR_INVALID, "block out rows: %d rows (at least 1)", n_rows);
    if (!span || n_blocks == 0 || n_blocks > 0x7fffffff) return fail(ctx, GDG_ERR_INVALID, "block out rows: %zu blocks, spans %s; 1 to 2^31 - 1 blocks need their spans", n_blocks, span ? "given" : "NULL");
    if (span[0] != 0 || span[n_blocks] != samples)
        return fail(ctx, GDG_ERR_INVALID, "block out rows: the spans run from %zu to %zu; they cover the rows' samples, 0 to %zu", span[0], span[n_blocks], samples);
    for (size_t k = 0; k < n_blocks; k++)
        if (span[k + 1] <= span[k] || span[k + 1] - span[k] > (size_t)GDG_OUT_RECORDS_MAX_BLOCK)
            return fail(ctx, GDG_ERR_INVALID, "block out rows: block %zu is the samples %zu to %zu; a block has 1 to %d samples and the spans ascend", k, span[k], span[k + 1],
                        GDG_OUT_RECORDS_MAX_BLOCK);
    return GDG_OK;
}

int gdg_block_out_rows_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, const size_t *span, size_t n_blocks, double *d_history,
                              gdg_block_delivered *d_records) {
    if (!ctx) return GDG_ERR_INVALID;
    const int rc = block_out_check(ctx, n_rows, samples, span, n_blocks);
    if (rc != GDG_OK) return rc;
    if (!d_rows || !d_records) return fail(ctx, GDG_ERR_INVALID, "block out rows: %s is NULL", !d_rows ? "the rows' pointer" : "the records' pointer");
    if (row_stride < samples) return fail(ctx, GDG_ERR_INVALID, "block out rows: a row stride of %zu samples for rows of %zu", row_stride, samples);
    if (((uintptr_t)d_rows & 7) || ((uintptr_t)d_records & 7) || ((uintptr_t)d_history & 7)) return fail(ctx, GDG_ERR_INVALID, "block out rows: rows, history and records are 8-byte aligned");
    enter_keep_fir_sums(ctx);
    /* the spans go up from the context's own copy: whatever the last call's launch still reads has to be done before either copy changes */
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const size_t bytes = (n_blocks + 1) * sizeof(unsigned long long);
    if (bytes > ctx->d_out_rows_spans_cap) {
        hipFree(ctx->d_out_rows_spans);
        ctx->d_out_rows_spans = nullptr;
        ctx->d_out_rows_spans_cap = 0;
        if (hipMalloc((void **)&ctx->d_out_rows_spans, bytes) != hipSuccess) return fail(ctx, GDG_ERR_NOMEM, "block out rows: cannot allocate the spans of %zu blocks on the device", n_blocks);
        ctx->d_out_rows_spans_cap = bytes;
    }
    ctx->out_rows_spans.assign(span, span + n_blocks + 1);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_out_rows_spans, ctx->out_rows_spans.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
    ProfScope ps(ctx, GDG_K_WAVE);
    HIP_TRY(ctx, gdg_launch_block_delivered(d_rows, row_stride, (unsigned)n_rows, samples, ctx->d_out_rows_spans, (unsigned)n_blocks, d_history, true_peak_table(), d_records, ctx->stream));
    /* behind the records: the last 23 samples of (history ++ rows) are what the next call finds in front of its own */
    if (d_history) HIP_TRY(ctx, gdg_launch_delivered_history_save(d_rows, row_stride, samples, (unsigned)n_rows, d_history, ctx->stream));
    return GDG_OK;
}

int gdg_block_out_rows(gdg_ctx *ctx, const double *const *rows, int n_rows, size_t samples, const size_t *span, size_t n_blocks, double *history, gdg_block_delivered *records) {
    if (!ctx) return GDG_ERR_INVALID;
    int rc = block_out_check(ctx, n_rows, samples, span, n_blocks);
    if (rc != GDG_OK) return rc;
    if (!rows || !records) return fail(ctx, GDG_ERR_INVALID, "block out rows: %s is NULL", !rows ? "the rows' list" : "the records' pointer");
    /* rows up into d_io[1] and records down from d_io[0] as the other kinds' go; the history, up before the launch and down behind it, takes a
     * buffer the call owns -- growing either d_io buffer now would move what is already enqueued */
    const size_t hist_bytes = history ? (size_t)n_rows * GDG_OUT_RECORDS_HISTORY * sizeof(double) : 0;
    return rows_round_trip(ctx, "block out rows", rows, n_rows, samples, records, (size_t)n_rows * n_blocks * sizeof(gdg_block_delivered), [&](const double *d_rows, void *d_out) {
        double *d_hist = nullptr;
        if (history) {
            if (hipMalloc((void **)&d_hist, hist_bytes) != hipSuccess) return fail(ctx, GDG_ERR_NOMEM, "block out rows: cannot allocate the history of %d rows on the device", n_rows);
            const hipError_t e = hipMemcpyAsync(d_hist, history, hist_bytes, hipMemcpyHostToDevice, ctx->stream);
            if (e != hipSuccess) { hipFree(d_hist); return fail(ctx, GDG_ERR_HIP, "block out rows: %s", hipGetErrorString(e)); }
        }
        int r = gdg_block_out_rows_device(ctx, d_rows, samples, n_rows, samples, span, n_blocks, d_hist, static_cast<gdg_block_delivered *>(d_out));
        if (d_hist) {
            if (r == GDG_OK && hipMemcpyAsync(history, d_hist, hist_bytes, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) r = GDG_ERR_HIP;
            hipStreamSynchronize(ctx->stream);
            hipFree(d_hist);
        }
        return r;
    });
}

/* capacity in records */
int gdg_batch_out_records(gdg_ctx *ctx, gdg_block_delivered *records, size_t capacity, int *ports, size_t *blocks) {
    static const ListWords words = { "no records of the delivered rows", "has not completed, was a master finish, or none has run since gdg_batch_out_records_enable",
                                     "ran without them (gdg_batch_out_records_enable comes before the call)", "out records", "records" };
    if (ctx && ports && ctx->list_rec[LIST_DELIVERED].valid) *ports = ctx->list_rec[LIST_DELIVERED].count;
    return batch_list_get(ctx, LIST_DELIVERED, words, records, capacity, blocks);
}
