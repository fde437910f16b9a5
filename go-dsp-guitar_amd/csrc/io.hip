/*
 * io.hip -- the data formats either side of the hot path:
 *   wave sample codecs  wave/wave.go:275-735   LPCM 8/16/24/32 and IEEE 32/64 <-> float64, bit exact
 *   resample.Time       resample/resample.go:72-103   Lanczos-3 rate conversion of whole files
 * Both are embarrassingly parallel and HBM bound (1..8 B in + 8 B out per sample for the codecs;
 * ~6 x 8 B gathered (cache hits) + 8 B out for the resampler, which is sin()-bound in FP64).
 */
#include "../../include/gdg.h"
#include "gdg_internal.h"
#include "dither.h"
#include "trim.h"
#include "blend.h"
#include <math.h>
#include <stdlib.h>

#define MAX_INT24 0x007fffff
#define MIN_INT24 (-(MAX_INT24 + 1))
#define SIGN_BIT_INT24 0x00800000

__device__ __forceinline__ double clamp1(double s) { return s < -1.0 ? -1.0 : (s > 1.0 ? 1.0 : s); }

template <int FMT>
__global__ void __launch_bounds__(256)
wave_decode_kernel(const unsigned char *__restrict__ data, size_t n, double *__restrict__ out, unsigned channels, size_t per) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        double r;
        if (FMT == GDG_FMT_LPCM8) {                              /* wave.go:316-342 */
            short temp = (short)((short)data[i] + (-128));
            r = (1.0 / 127.0) * (double)temp;
            r = r < -1.0 ? -1.0 : (r > 1.0 ? 1.0 : r);
        } else if (FMT == GDG_FMT_LPCM16) {                      /* wave.go:400-428 */
            short s = (short)(unsigned short)(data[2 * i] | (data[2 * i + 1] << 8));
            r = (2.0 / 65535.0) * (double)s;
        } else if (FMT == GDG_FMT_LPCM24) {                      /* wave.go:483-531 */
            unsigned w = (unsigned)data[3 * i] | ((unsigned)data[3 * i + 1] << 8) | ((unsigned)data[3 * i + 2] << 16);
            int v = (int)w;
            if (w & SIGN_BIT_INT24) v = MIN_INT24 + (v & MAX_INT24);
            r = (2.0 / 16777215.0) * (double)v;
        } else if (FMT == GDG_FMT_LPCM32) {                      /* wave.go:589-617 */
            unsigned w = reinterpret_cast<const unsigned *>(data)[i];
            r = (2.0 / 4294967295.0) * (double)(int)w;
        } else if (FMT == GDG_FMT_IEEE32) {                      /* wave.go:662-689 */
            r = (double)reinterpret_cast<const float *>(data)[i];
        } else {                                                 /* wave.go:714-732 */
            r = reinterpret_cast<const double *>(data)[i];
        }
        /* samplesToChannels (wave.go:237-270): interleaved sample i belongs to channel i % C, position i / C */
        out[channels == 1 ? i : (size_t)(i % channels) * per + i / channels] = r;
    }
}

template <int FMT>
__global__ void __launch_bounds__(256)
wave_encode_kernel(const double *__restrict__ in, size_t n, unsigned char *__restrict__ data, unsigned channels, size_t per) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        /* channelsToSamples (wave.go:173-232) */
        double sample = in[channels == 1 ? i : (size_t)(i % channels) * per + i / channels];
        if (FMT == GDG_FMT_LPCM8) {                              /* wave.go:275-311 */
            sample = clamp1(sample);
            short temp = (short)(127.0 * sample);
            int res = temp + 128;
            data[i] = (unsigned char)(res < 0 ? 0 : (res > 255 ? 255 : res));
        } else if (FMT == GDG_FMT_LPCM16) {                      /* wave.go:347-395 */
            sample = clamp1(sample);
            int tmp = (int)((0.5 * 65535.0) * sample);
            tmp = tmp > 32767 ? 32767 : (tmp < -32768 ? -32768 : tmp);
            reinterpret_cast<short *>(data)[i] = (short)tmp;
        } else if (FMT == GDG_FMT_LPCM24) {                      /* wave.go:433-478 */
            sample = clamp1(sample);
            int tmp = (int)((0.5 * 16777215.0) * sample);
            tmp = tmp > MAX_INT24 ? MAX_INT24 : (tmp < MIN_INT24 ? MIN_INT24 : tmp);
            unsigned u = (unsigned)tmp;
            data[3 * i] = (unsigned char)(u & 0xff);
            data[3 * i + 1] = (unsigned char)((u >> 8) & 0xff);
            data[3 * i + 2] = (unsigned char)((u >> 16) & 0xff);
        } else if (FMT == GDG_FMT_LPCM32) {                      /* wave.go:536-584 */
            sample = clamp1(sample);
            long long tmp = (long long)((0.5 * 4294967295.0) * sample);
            tmp = tmp > 2147483647LL ? 2147483647LL : (tmp < -2147483648LL ? -2147483648LL : tmp);
            reinterpret_cast<int *>(data)[i] = (int)tmp;
        } else if (FMT == GDG_FMT_IEEE32) {                      /* wave.go:622-657 */
            reinterpret_cast<float *>(data)[i] = (float)clamp1(sample);
        } else {                                                 /* wave.go:694-709: no clipping */
            reinterpret_cast<double *>(data)[i] = sample;
        }
    }
}

/* resample/resample.go:10-31 */
__device__ __forceinline__ double lanczos_kernel(double x, double a) {
    if (x == 0) return 1.0;
    if ((-a < x) && (x < a)) {
        double pi_x = M_PI * x;
        double pi_xa = pi_x / a;
        double pi_x_squared = pi_x * pi_x;
        double prod = sin(pi_x) * sin(pi_xa);
        double arg = a * prod;
        return arg / pi_x_squared;
    }
    return 0.0;
}

/* resample.Time: out[i] = sum_{j = floor(x)-2}^{floor(x)+3} s[j] L3(x - j), x = i * (src / dst) (resample.go:36-103) */
__global__ void __launch_bounds__(256)
resample_time_kernel(const double *__restrict__ s, int n, double dx, double *__restrict__ out, int n_out) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n_out; i += gridDim.x * 256) {
        double x = (double)i * dx;
        int idx = (int)floor(x);
        double sum = 0.0;
#pragma unroll
        for (int j = idx - 2; j < idx + 4; j++) {
            if (j >= 0 && j < n) {
                double diff = x - (double)j;
                sum += s[j] * lanczos_kernel(diff, 3.0);
            }
        }
        out[i] = sum;
    }
}

/* ------------------------------------------------------------------------------------------------
 * level/level.go:147-210 channel meter, one workgroup per port, at most GDG_METER_SEG samples per launch.
 *   current:  c <- max(c * d, |x|)  ==  max(c0 d^n, max_i |x_i| d^(n-1-i))            (weighted max reduction)
 *   peak/hold: the reference's per-sample state machine (decay once the counter passed `hold`, a sample
 *   >= peak records and restarts the hold) has, within a segment of n <= hold samples, exactly one
 *   interesting event: the FIRST record r.  Before it the peak is p0 (hold phase) or p0 d^k (decay phase,
 *   closed form); after it the peak is the running maximum of |x_r..|, the counter the distance to the LAST
 *   sample attaining that maximum.  The host guarantees n <= hold (gdg_meter_process splits).
 * ---------------------------------------------------------------------------------------------- */
#define METER_T 1024
#define METER_CHK (GDG_METER_SEG / METER_T)

/* Two values reduced over the workgroup in one go: the maximum of `v` and the maximum of the pair (key, idx) in the order "larger key, then
 * larger idx".  Wave level by shuffles, the 16 wave results through LDS, and EVERY wave finishes the reduction from those 16 cells with four
 * more shuffle steps (no serial walk over the partials: that walk alone was ~1 000 cycles, and the kernel had four such reductions). */
struct MeterRed { double v; double key; int idx; };
__device__ __forceinline__ MeterRed meter_reduce(MeterRed x, double *scr_v, double *scr_k, int *scr_i) {
    const int tid = threadIdx.x, lane = tid & 63;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_down(x.v, o), ok = __shfl_down(x.key, o);
        const int oi = __shfl_down(x.idx, o);
        x.v = fmax(x.v, ov);
        if (ok > x.key || (ok == x.key && oi > x.idx)) { x.key = ok; x.idx = oi; }
    }
    __syncthreads();                                    /* the cells of the reduction before are no longer read */
    if (lane == 0) { scr_v[tid >> 6] = x.v; scr_k[tid >> 6] = x.key; scr_i[tid >> 6] = x.idx; }
    __syncthreads();
    MeterRed r = { scr_v[lane & 15], scr_k[lane & 15], scr_i[lane & 15] };
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
        const double ov = __shfl_xor(r.v, o), ok = __shfl_xor(r.key, o);
        const int oi = __shfl_xor(r.idx, o);
        r.v = fmax(r.v, ov);
        if (ok > r.key || (ok == r.key && oi > r.idx)) { r.key = ok; r.idx = oi; }
    }
    return r;
}
static_assert(METER_T / 64 == 16, "meter_reduce finishes from 16 wave results");

__global__ void __launch_bounds__(METER_T)
meter_kernel(const double *__restrict__ rows, size_t stride, int n, gdg_meter_rec *__restrict__ st,
             double decay, unsigned long long hold) {
    __shared__ double scr_v[METER_T / 64], scr_k[METER_T / 64];
    __shared__ int scr_i[METER_T / 64];
    /* a thread works on METER_CHK CONSECUTIVE samples (the follower is sequential inside a chunk), but the port is read the way memory
     * likes it -- lane after lane, all loads of the thread in flight -- and turned through LDS (one pad cell per 32, as in the segment
     * kernel).  Reading x[base + k] directly gave every lane its own 64-byte piece of a 4 KiB span per instruction: eight times the
     * port's bytes between L2 and L1. */
    __shared__ double turn[GDG_METER_SEG + GDG_METER_SEG / 32];
    /* decay^m for the exponents the closed forms need (0 <= m <= n <= 8192): three small tables made by 73 threads with pow(), every
     * other power is a product of three entries (pow() in every thread, three calls of ~300 FP64 instructions each, kept all SIMDs busy
     * for ~11 us per round of 256 workgroups). */
    __shared__ double pw_lo[32], pw_hi[33], pw_one[8];      /* (d^8)^j, (d^256)^i, d^j */
    const int tid = threadIdx.x;
    gdg_meter_rec *m = st + blockIdx.x;
    const double *x = rows + (size_t)blockIdx.x * stride;
    /* a disabled port's row is never touched: gdg_meter_process_device takes caller-supplied rows, and a caller may leave the rows of
     * disabled ports unbacked (`enabled` is uniform over the workgroup: one scalar load in front of the row loads) */
    if (!m->enabled) return;
    double t[METER_CHK];
#pragma unroll
    for (int k = 0; k < METER_CHK; k++) { const int i = tid + METER_T * k; t[k] = (i < n) ? x[i] : 0.0; }     /* in flight while the tables are made */
    const double c0 = m->current, p0 = m->peak;
    const unsigned long long cnt0 = m->counter;
    const int base = tid * METER_CHK;
    if (tid < 32) pw_lo[tid] = pow(decay, (double)(8 * tid));
    else if (tid < 65) pw_hi[tid - 32] = pow(decay, (double)(256 * (tid - 32)));
    else if (tid < 73) pw_one[tid - 65] = pow(decay, (double)(tid - 65));
#pragma unroll
    for (int k = 0; k < METER_CHK; k++) { const int i = tid + METER_T * k; turn[i + (i >> 5)] = t[k]; }
    __syncthreads();
    auto dpow = [&](long long e) -> double {                /* 0 <= e <= 8192 + 7 */
        const int a8 = (int)(e >> 3);
        return (pw_hi[a8 >> 5] * pw_lo[a8 & 31]) * pw_one[(int)(e & 7)];
    };
    double a[METER_CHK];
#pragma unroll
    for (int k = 0; k < METER_CHK; k++) { const int i = base + k; a[k] = (i < n) ? fabs(turn[i + (i >> 5)]) : -1.0; }

    /* current value: zero-state follower over the chunk, then its decay to the end of the segment */
    double b = 0.0;
    int len = 0;
#pragma unroll
    for (int k = 0; k < METER_CHK; k++)
        if (base + k < n) { b *= decay; if (a[k] > b) b = a[k]; len++; }
    const double contrib = (len > 0) ? b * dpow(n - base - len) : 0.0;

    /* first record: smallest i with |x_i| >= p_i;  p_i = p0 for i < e, p0 d^(i-e+1) from e on */
    const long long e = (cnt0 > hold) ? 0 : (long long)(hold - cnt0) + 1;
    double p = p0;
    if ((long long)base >= e) p = p0 * dpow((long long)base - e);      /* value before sample `base` decays */
    int first = n;
#pragma unroll
    for (int k = 0; k < METER_CHK; k++) {
        int i = base + k;
        if (i < n) {
            if ((long long)i >= e) p *= decay;
            if (first == n && a[k] >= p) first = i;
        }
    }
    /* one reduction for both: the largest contribution, and the smallest `first` (as the largest n - first) */
    const MeterRed r1 = meter_reduce(MeterRed{ contrib, 0.0, n - first }, scr_v, scr_k, scr_i);
    const double cur = fmax(r1.v, c0 * dpow(n));
    const int r = n - r1.idx;

    double peak;
    unsigned long long counter;
    if (r >= n) {       /* no record in this segment */
        long long dec = (long long)n - e;
        peak = (dec > 0) ? p0 * dpow(dec) : p0;
        counter = (cnt0 > hold) ? cnt0 : ((cnt0 + (unsigned long long)n < hold + 1) ? cnt0 + (unsigned long long)n : hold + 1);
    } else {
        /* from the record on the peak is the running maximum, the counter the distance to the LAST sample attaining it: the pair
         * (value, index) reduced in the order "larger value, then larger index" */
        double mx = -1.0;
        int last = -1;
#pragma unroll
        for (int k = 0; k < METER_CHK; k++)
            if (base + k >= r && base + k < n && a[k] >= mx) { mx = a[k]; last = base + k; }
        const MeterRed r2 = meter_reduce(MeterRed{ 0.0, mx, last }, scr_v, scr_k, scr_i);
        peak = r2.key;
        counter = (unsigned long long)(n - 1 - r2.idx);
    }
    if (tid == 0) { m->current = cur; m->peak = peak; m->counter = counter; }
}

hipError_t gdg_launch_meter(const double *d_rows, size_t stride, int n_ports, int n, gdg_meter_rec *d_state,
                            double decay, unsigned long long hold, hipStream_t s) {
    if (n_ports <= 0 || n <= 0) return hipSuccess;
    if (n > GDG_METER_SEG) return hipErrorInvalidValue;
    meter_kernel<<<n_ports, METER_T, 0, s>>>(d_rows, stride, n, d_state, decay, hold);
    return hipGetLastError();
}

/* ------------------------------------------------------------------------------------------------
 * metronome/metronome.go:63-131.  The two counters have closed forms inside a buffer: up to and including sample j0 (the
 * last one before the first beat boundary) the sample counter is sc0 + i; after it sample i lies m = i - j0 - 1 samples
 * into a run of whole beats: counter = m mod spb, resets so far = 1 + m div spb.  The host keeps the two counters.
 * ---------------------------------------------------------------------------------------------- */
__global__ void __launch_bounds__(256)
metronome_kernel(const double *__restrict__ tick, unsigned n_tick, const double *__restrict__ tock, unsigned n_tock, double *__restrict__ out, int n,
                 unsigned sc0, unsigned tc0, unsigned spb, unsigned beats, unsigned j0) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        unsigned sc, tc;
        if ((unsigned)i <= j0) { sc = sc0 + (unsigned)i; tc = tc0; }
        else {
            unsigned m = (unsigned)i - j0 - 1u;
            unsigned resets = 1u + (spb ? m / spb : m);
            sc = spb ? m % spb : 0u;
            tc = ((tc0 + 1u) % beats + (resets - 1u) % beats) % beats;
        }
        double sample = 0.0;
        if (tc == 0) { if (tick && sc < n_tick) sample = tick[sc]; }
        else { if (tock && sc < n_tock) sample = tock[sc]; }
        out[i] = sample;
    }
}

__global__ void __launch_bounds__(256) add_aux_kernel(double *__restrict__ a, double *__restrict__ b, const double *__restrict__ src, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) { const double v = src[i]; a[i] += v; b[i] += v; }
}
hipError_t gdg_launch_add_aux(double *d_a, double *d_b, const double *d_src, int n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    add_aux_kernel<<<(n + 255) / 256, 256, 0, s>>>(d_a, d_b, d_src, n);
    return hipGetLastError();
}

hipError_t gdg_launch_metronome(const double *d_tick, unsigned n_tick, const double *d_tock, unsigned n_tock, double *d_out, int n,
                                unsigned sc0, unsigned tc0, unsigned spb, unsigned beats, unsigned j0, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    metronome_kernel<<<(n + 255) / 256, 256, 0, s>>>(d_tick, n_tick, d_tock, n_tock, d_out, n, sc0, tc0, spb, beats, j0);
    return hipGetLastError();
}

static int grid_for(size_t n) {
    size_t blocks = (n + 255) / 256;
    if (blocks > 256 * 8) blocks = 256 * 8;
    return (int)(blocks ? blocks : 1);
}

/* ---- mono fast path: four samples per thread, word-sized loads and stores ---------------------------------------- */
template <int FMT> struct fmt_width { static const int W = FMT == GDG_FMT_LPCM8 ? 1 : FMT == GDG_FMT_LPCM16 ? 2 : FMT == GDG_FMT_LPCM24 ? 3 : 4; };
/* STMT once with FMT a constant: every format (GDG_DISPATCH_FMT) or the four LPCM ones (GDG_DISPATCH_LPCM); any other value is refused */
#define GDG_FMT_CASE(F, STMT) case F: { constexpr int FMT = F; STMT; break; }
#define GDG_LPCM_CASES(STMT) GDG_FMT_CASE(GDG_FMT_LPCM8, STMT) GDG_FMT_CASE(GDG_FMT_LPCM16, STMT) GDG_FMT_CASE(GDG_FMT_LPCM24, STMT) GDG_FMT_CASE(GDG_FMT_LPCM32, STMT)
#define GDG_DISPATCH_LPCM(F, STMT) switch (F) { GDG_LPCM_CASES(STMT) default: return hipErrorInvalidValue; }
#define GDG_DISPATCH_FMT(F, STMT) \
    switch (F) { GDG_LPCM_CASES(STMT) GDG_FMT_CASE(GDG_FMT_IEEE32, STMT) GDG_FMT_CASE(GDG_FMT_IEEE64, STMT) default: return hipErrorInvalidValue; }
__device__ __forceinline__ unsigned getb(const unsigned *w, int k) { return (w[k >> 2] >> ((k & 3) * 8)) & 0xffu; }

template <int FMT>
__device__ __forceinline__ double decode_code(unsigned code) {       /* code = the sample's little-endian bytes */
    if (FMT == GDG_FMT_LPCM8) {
        short temp = (short)((short)code + (-128));
        double r = (1.0 / 127.0) * (double)temp;
        return r < -1.0 ? -1.0 : (r > 1.0 ? 1.0 : r);
    } else if (FMT == GDG_FMT_LPCM16) {
        return (2.0 / 65535.0) * (double)(short)(unsigned short)code;
    } else if (FMT == GDG_FMT_LPCM24) {
        int v = (int)code;
        if (code & SIGN_BIT_INT24) v = MIN_INT24 + (v & MAX_INT24);
        return (2.0 / 16777215.0) * (double)v;
    } else if (FMT == GDG_FMT_LPCM32) {
        return (2.0 / 4294967295.0) * (double)(int)code;
    } else {
        return (double)__uint_as_float(code);
    }
}

template <int FMT>
__device__ __forceinline__ unsigned encode_code(double sample) {
    sample = clamp1(sample);
    if (FMT == GDG_FMT_LPCM8) {
        short temp = (short)(127.0 * sample);
        int res = temp + 128;
        return (unsigned)(res < 0 ? 0 : (res > 255 ? 255 : res));
    } else if (FMT == GDG_FMT_LPCM16) {
        int tmp = (int)((0.5 * 65535.0) * sample);
        tmp = tmp > 32767 ? 32767 : (tmp < -32768 ? -32768 : tmp);
        return (unsigned)tmp & 0xffffu;
    } else if (FMT == GDG_FMT_LPCM24) {
        int tmp = (int)((0.5 * 16777215.0) * sample);
        tmp = tmp > MAX_INT24 ? MAX_INT24 : (tmp < MIN_INT24 ? MIN_INT24 : tmp);
        return (unsigned)tmp & 0xffffffu;
    } else if (FMT == GDG_FMT_LPCM32) {
        long long tmp = (long long)((0.5 * 4294967295.0) * sample);
        tmp = tmp > 2147483647LL ? 2147483647LL : (tmp < -2147483648LL ? -2147483648LL : tmp);
        return (unsigned)(int)tmp;
    } else {
        return __float_as_uint((float)sample);
    }
}

typedef double v2d __attribute__((ext_vector_type(2)));

template <int FMT, bool NT>
__global__ void __launch_bounds__(256)
wave_decode4_kernel(const unsigned *__restrict__ words, size_t groups, v2d *__restrict__ out) {
    constexpr int W = fmt_width<FMT>::W;
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (size_t)gridDim.x * 256) {
        unsigned w[W];
#pragma unroll
        for (int k = 0; k < W; k++) w[k] = NT ? __builtin_nontemporal_load(words + g * W + k) : words[g * W + k];
        double r[4];
#pragma unroll
        for (int s = 0; s < 4; s++) {
            unsigned code = 0;
#pragma unroll
            for (int k = 0; k < W; k++) code |= getb(w, s * W + k) << (8 * k);
            r[s] = decode_code<FMT>(code);
        }
        v2d a = { r[0], r[1] }, b = { r[2], r[3] };
        if (NT) { __builtin_nontemporal_store(a, out + 2 * g); __builtin_nontemporal_store(b, out + 2 * g + 1); }
        else { out[2 * g] = a; out[2 * g + 1] = b; }
    }
}

template <int FMT>
static void launch_decode(const unsigned char *p, size_t per, unsigned channels, double *d_out, hipStream_t s) {
    size_t n = per * channels, done = 0;
    if (FMT != GDG_FMT_IEEE64 && channels == 1 && n >= 4 && ((uintptr_t)p & 3) == 0 && ((uintptr_t)d_out & 15) == 0) {
        size_t groups = n / 4;
        /* measured (profiles/io_variants_r01.txt): one group per thread without a grid cap; plain stores for decode, non-temporal for encode */
        wave_decode4_kernel<FMT, false><<<(unsigned)((groups + 255) / 256), 256, 0, s>>>(reinterpret_cast<const unsigned *>(p), groups, reinterpret_cast<v2d *>(d_out));
        done = groups * 4;
    }
    if (done < n) {         /* tail, multi-channel files, unaligned buffers: the one-sample-per-thread kernel */
        size_t off = done * gdg_wave_bytes_per_sample(FMT);
        if (channels == 1) wave_decode_kernel<FMT><<<grid_for(n - done), 256, 0, s>>>(p + off, n - done, d_out + done, 1, n - done);
        else wave_decode_kernel<FMT><<<grid_for(n), 256, 0, s>>>(p, n, d_out, channels, per);
    }
}

template <int FMT>
__device__ __forceinline__ void decode_piece(const gdg_decode_row &r) {
    constexpr int W = fmt_width<FMT>::W;
    unsigned done = 0;
    if ((((uintptr_t)r.src) & 3) == 0 && (((uintptr_t)r.dst) & 15) == 0) {
        /* word-sized loads, four samples per thread: byte loads fetch every line W times over (the batch run's pieces are 16-byte aligned) */
        const unsigned *words = reinterpret_cast<const unsigned *>(r.src);
        v2d *out = reinterpret_cast<v2d *>(r.dst);
        const unsigned groups = r.count / 4;
        for (unsigned g = blockIdx.x * 256 + threadIdx.x; g < groups; g += gridDim.x * 256) {
            unsigned w[W];
#pragma unroll
            for (int k = 0; k < W; k++) w[k] = __builtin_nontemporal_load(words + (size_t)g * W + k);
            double v[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                unsigned code = 0;
#pragma unroll
                for (int k = 0; k < W; k++) code |= getb(w, q * W + k) << (8 * k);
                v[q] = decode_code<FMT>(code);
            }
            v2d a = { v[0], v[1] }, b = { v[2], v[3] };
            out[2 * (size_t)g] = a;
            out[2 * (size_t)g + 1] = b;
        }
        done = groups * 4;
    }
    for (unsigned i = done + blockIdx.x * 256 + threadIdx.x; i < r.count; i += gridDim.x * 256) {
        unsigned code = 0;
#pragma unroll
        for (int k = 0; k < W; k++) code |= (unsigned)r.src[(size_t)i * W + k] << (8 * k);
        r.dst[i] = decode_code<FMT>(code);
    }
}

/* a piece that picks one channel out of interleaved frames (samplesToChannels, wave.go:237-270, for that channel alone): sample i is the
 * file's sample i * stride + offset.  One sample per thread, byte loads: neighbouring lanes read `stride` samples apart. */
template <int FMT>
__device__ __forceinline__ void decode_piece_strided(const gdg_decode_row &r) {
    constexpr int W = fmt_width<FMT>::W;
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < r.count; i += gridDim.x * 256) {
        const size_t at = ((size_t)i * r.stride + r.offset) * W;
        unsigned code = 0;
#pragma unroll
        for (int k = 0; k < W; k++) code |= (unsigned)r.src[at + k] << (8 * k);
        r.dst[i] = decode_code<FMT>(code);
    }
}

/* blockIdx.y = piece; every piece has its own format (uniform per workgroup), source and destination */
__global__ void __launch_bounds__(256)
wave_decode_rows_kernel(const gdg_decode_row *__restrict__ rows) {
    const gdg_decode_row r = rows[blockIdx.y];
    if (r.stride > 1) {                                        /* a channel of an interleaved file (the streamed batch run) */
        switch (r.fmt) {
        case GDG_FMT_LPCM8: decode_piece_strided<GDG_FMT_LPCM8>(r); break;
        case GDG_FMT_LPCM16: decode_piece_strided<GDG_FMT_LPCM16>(r); break;
        case GDG_FMT_LPCM24: decode_piece_strided<GDG_FMT_LPCM24>(r); break;
        case GDG_FMT_LPCM32: decode_piece_strided<GDG_FMT_LPCM32>(r); break;
        case GDG_FMT_IEEE32: decode_piece_strided<GDG_FMT_IEEE32>(r); break;
        default:
            for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < r.count; i += gridDim.x * 256)
                r.dst[i] = reinterpret_cast<const double *>(r.src)[(size_t)i * r.stride + r.offset];
            break;
        }
        return;
    }
    switch (r.fmt) {
    case GDG_FMT_LPCM8: decode_piece<GDG_FMT_LPCM8>(r); break;
    case GDG_FMT_LPCM16: decode_piece<GDG_FMT_LPCM16>(r); break;
    case GDG_FMT_LPCM24: decode_piece<GDG_FMT_LPCM24>(r); break;
    case GDG_FMT_LPCM32: decode_piece<GDG_FMT_LPCM32>(r); break;
    case GDG_FMT_IEEE32: decode_piece<GDG_FMT_IEEE32>(r); break;
    default:                                                   /* IEEE64 (wave.go:714-732): the bytes are the sample; src is 8-byte aligned */
        for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < r.count; i += gridDim.x * 256) r.dst[i] = reinterpret_cast<const double *>(r.src)[i];
        break;
    }
}

hipError_t gdg_launch_wave_decode_rows(const gdg_decode_row *d_rows, int n_rows, unsigned max_count, hipStream_t s) {
    if (n_rows <= 0 || max_count == 0) return hipSuccess;
    unsigned tiles = (max_count + 1023) / 1024;                /* four samples per thread */
    if (tiles > 64) tiles = 64;
    wave_decode_rows_kernel<<<dim3(tiles, (unsigned)n_rows), dim3(256), 0, s>>>(d_rows);
    return hipGetLastError();
}

/* ---- the fan-out form: a piece decoded once, stored to every row of its fan (a batch job with a source map) ------------------------------ */
/* the four samples of group g through word-sized loads, as decode_piece's fast path reads them */
template <int FMT>
__device__ __forceinline__ void decode_group(const unsigned *words, unsigned g, double v[4]) {
    constexpr int W = fmt_width<FMT>::W;
    unsigned w[W];
#pragma unroll
    for (int k = 0; k < W; k++) w[k] = __builtin_nontemporal_load(words + (size_t)g * W + k);
#pragma unroll
    for (int q = 0; q < 4; q++) {
        unsigned code = 0;
#pragma unroll
        for (int k = 0; k < W; k++) code |= getb(w, q * W + k) << (8 * k);
        v[q] = decode_code<FMT>(code);
    }
}
/* the file's sample `at` through byte loads (tails, unaligned pieces, a channel of interleaved frames) */
template <int FMT>
__device__ __forceinline__ double decode_at(const unsigned char *src, size_t at) {
    constexpr int W = fmt_width<FMT>::W;
    unsigned code = 0;
#pragma unroll
    for (int k = 0; k < W; k++) code |= (unsigned)src[at * W + k] << (8 * k);
    return decode_code<FMT>(code);
}

/* blockIdx.y = fan.  The format switch yields values in registers; the loop over the fan's rows lies outside it, and in it consecutive
 * lanes store consecutive samples of ONE row before the next row (rows of a slice lie a slice apart).  No workgroup waits for another. */
__global__ void __launch_bounds__(256)
wave_decode_fans_kernel(const gdg_decode_fan *__restrict__ fans, double *const *__restrict__ table) {
    const gdg_decode_fan r = fans[blockIdx.y];
    double *const *rows = table + r.dst_first;
    unsigned done = 0;
    if (r.stride <= 1 && r.fmt != GDG_FMT_IEEE64 && r.vec && (((uintptr_t)r.src) & 3) == 0) {
        const unsigned *words = reinterpret_cast<const unsigned *>(r.src);
        const unsigned groups = r.count / 4;
        for (unsigned g = blockIdx.x * 256 + threadIdx.x; g < groups; g += gridDim.x * 256) {
            double v[4];
            switch (r.fmt) {
            case GDG_FMT_LPCM8: decode_group<GDG_FMT_LPCM8>(words, g, v); break;
            case GDG_FMT_LPCM16: decode_group<GDG_FMT_LPCM16>(words, g, v); break;
            case GDG_FMT_LPCM24: decode_group<GDG_FMT_LPCM24>(words, g, v); break;
            case GDG_FMT_LPCM32: decode_group<GDG_FMT_LPCM32>(words, g, v); break;
            default: decode_group<GDG_FMT_IEEE32>(words, g, v); break;
            }
            const v2d a = { v[0], v[1] }, b = { v[2], v[3] };
            for (unsigned d = 0; d < r.n_dst; d++) {
                v2d *out = reinterpret_cast<v2d *>(rows[d]);
                out[2 * (size_t)g] = a;
                out[2 * (size_t)g + 1] = b;
            }
        }
        done = groups * 4;
    }
    for (unsigned i = done + blockIdx.x * 256 + threadIdx.x; i < r.count; i += gridDim.x * 256) {
        const size_t at = r.stride > 1 ? (size_t)i * r.stride + r.offset : (size_t)i;
        double v;
        switch (r.fmt) {
        case GDG_FMT_LPCM8: v = decode_at<GDG_FMT_LPCM8>(r.src, at); break;
        case GDG_FMT_LPCM16: v = decode_at<GDG_FMT_LPCM16>(r.src, at); break;
        case GDG_FMT_LPCM24: v = decode_at<GDG_FMT_LPCM24>(r.src, at); break;
        case GDG_FMT_LPCM32: v = decode_at<GDG_FMT_LPCM32>(r.src, at); break;
        case GDG_FMT_IEEE32: v = decode_at<GDG_FMT_IEEE32>(r.src, at); break;
        default: v = reinterpret_cast<const double *>(r.src)[at]; break;      /* IEEE64: the bytes are the sample; src is 8-byte aligned */
        }
        for (unsigned d = 0; d < r.n_dst; d++) rows[d][i] = v;
    }
}

hipError_t gdg_launch_wave_decode_fans(const gdg_decode_fan *d_fans, double *const *d_table, int n_fans, unsigned max_count, hipStream_t s) {
    if (n_fans <= 0 || max_count == 0) return hipSuccess;
    unsigned tiles = (max_count + 1023) / 1024;                /* four samples per thread */
    if (tiles > 256) tiles = 256;                              /* a thread's stores grow with its fan: more workgroups than the single-row launch */
    wave_decode_fans_kernel<<<dim3(tiles, (unsigned)n_fans), dim3(256), 0, s>>>(d_fans, d_table);
    return hipGetLastError();
}

hipError_t gdg_launch_wave_decode(int fmt, const void *d_bytes, size_t per, unsigned channels, double *d_out, hipStream_t s) {
    size_t n = per * channels;
    if (n == 0) return hipSuccess;
    const unsigned char *p = static_cast<const unsigned char *>(d_bytes);
    GDG_DISPATCH_FMT(fmt, launch_decode<FMT>(p, per, channels, d_out, s));
    return hipGetLastError();
}

/* the stand-alone mono form's aligned bulk: one group per thread without a grid cap, non-temporal loads and stores (measured,
 * profiles/io_variants_r01.txt) */
template <int FMT>
__global__ void __launch_bounds__(256)
wave_encode4_kernel(const v2d *__restrict__ in, size_t groups, unsigned *__restrict__ words) {
    constexpr int W = fmt_width<FMT>::W;
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (size_t)gridDim.x * 256) {
        v2d a = __builtin_nontemporal_load(in + 2 * g), b = __builtin_nontemporal_load(in + 2 * g + 1);
        double r[4] = { a.x, a.y, b.x, b.y };
        unsigned w[W];
#pragma unroll
        for (int k = 0; k < W; k++) w[k] = 0;
#pragma unroll
        for (int s = 0; s < 4; s++) {
            unsigned code = encode_code<FMT>(r[s]);
#pragma unroll
            for (int k = 0; k < W; k++) {
                int byte = s * W + k;
                w[byte >> 2] |= ((code >> (8 * k)) & 0xffu) << ((byte & 3) * 8);
            }
        }
#pragma unroll
        for (int k = 0; k < W; k++) __builtin_nontemporal_store(w[k], words + g * W + k);
    }
}

/* n_rows rows of row_len samples each, row r at d_in + r * row_stride, encoded into COMPACT rows of row_len * width bytes: the batch
 * run's window keeps one row stride for every step (full windows and the tail), so one plan serves the whole batch; blockIdx.y = row.
 * row_len a multiple of 4, rows 16-byte aligned (the batch run's rows are multiples of 8192 samples). */
template <int FMT>
__global__ void __launch_bounds__(256)
wave_encode4_rows_kernel(const double *__restrict__ in, size_t row_stride, size_t groups_per_row, unsigned *__restrict__ words) {
    constexpr int W = fmt_width<FMT>::W;
    const v2d *row = reinterpret_cast<const v2d *>(in + (size_t)blockIdx.y * row_stride);
    unsigned *dst = words + (size_t)blockIdx.y * groups_per_row * W;
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups_per_row; g += (size_t)gridDim.x * 256) {
        v2d a = __builtin_nontemporal_load(row + 2 * g), b = __builtin_nontemporal_load(row + 2 * g + 1);
        double r[4] = { a.x, a.y, b.x, b.y };
        unsigned w[W];
#pragma unroll
        for (int k = 0; k < W; k++) w[k] = 0;
#pragma unroll
        for (int s = 0; s < 4; s++) {
            unsigned code = encode_code<FMT>(r[s]);
#pragma unroll
            for (int k = 0; k < W; k++) {
                int byte = s * W + k;
                w[byte >> 2] |= ((code >> (8 * k)) & 0xffu) << ((byte & 3) * 8);
            }
        }
#pragma unroll
        for (int k = 0; k < W; k++) __builtin_nontemporal_store(w[k], dst + g * W + k);
    }
}

/* The master of one piece of a sharded job in ONE launch (gdg_batch_finish_master and _slice): the slab holds G left rows, G right rows and
 * the aux row, `stride` samples apart.  A thread takes four consecutive samples of both sides: p_0, then + p_1 .. + p_{G-1} in shard order,
 * then + aux -- one IEEE add after the other, never contracted, so the bits of that order wherever it is computed -- and encodes them into
 * whole words as wave_encode4_kernel does (IEEE64: the sums are the bytes, wave.go:694-709).  Every partial is read once and never again:
 * non-temporal loads, and non-temporal stores for what goes straight down the bus.  SUMS: the float64 sums stay for the meters. */
template <int FMT, bool SUMS>
__global__ void __launch_bounds__(256)
finish_master_kernel(const double *__restrict__ slab, size_t stride, int G, int has_aux, size_t groups, unsigned *__restrict__ words_left,
                     unsigned *__restrict__ words_right, double *__restrict__ sums, size_t sums_stride) {
    constexpr int W = fmt_width<FMT>::W;
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= groups) return;
    const size_t rs = stride / 2;                                  /* v2d per row */
    const v2d *col = reinterpret_cast<const v2d *>(slab) + 2 * g;
    v2d xa = { 0.0, 0.0 }, xb = { 0.0, 0.0 };
    if (has_aux) { const v2d *q = col + (size_t)(2 * G) * rs; xa = __builtin_nontemporal_load(q); xb = __builtin_nontemporal_load(q + 1); }
#pragma unroll
    for (int side = 0; side < 2; side++) {
        const v2d *p = col + (size_t)(side * G) * rs;
        v2d a = __builtin_nontemporal_load(p), b = __builtin_nontemporal_load(p + 1);
#pragma unroll 4
        for (int k = 1; k < G; k++) {
            p += rs;
            a += __builtin_nontemporal_load(p);
            b += __builtin_nontemporal_load(p + 1);
        }
        if (has_aux) { a += xa; b += xb; }
        if (SUMS) {
            v2d *out = reinterpret_cast<v2d *>(sums + (size_t)side * sums_stride) + 2 * g;
            out[0] = a;
            out[1] = b;
        }
        unsigned *words = side ? words_right : words_left;
        if (!words) continue;
        if (FMT == GDG_FMT_IEEE64) {
            v2d *out = reinterpret_cast<v2d *>(words) + 2 * g;
            __builtin_nontemporal_store(a, out);
            __builtin_nontemporal_store(b, out + 1);
        } else {
            const double r[4] = { a.x, a.y, b.x, b.y };
            unsigned w[W];
#pragma unroll
            for (int k = 0; k < W; k++) w[k] = 0;
#pragma unroll
            for (int s = 0; s < 4; s++) {
                unsigned code = encode_code<FMT>(r[s]);
#pragma unroll
                for (int k = 0; k < W; k++) {
                    int byte = s * W + k;
                    w[byte >> 2] |= ((code >> (8 * k)) & 0xffu) << ((byte & 3) * 8);
                }
            }
#pragma unroll
            for (int k = 0; k < W; k++) __builtin_nontemporal_store(w[k], words + g * W + k);
        }
    }
}

/* ------------------------------------------------------------------------------------------------
 * The dithered encoders (dither.h; include/gdg.h, gdg_batch_set_dither): TPDF dither with rounding for the four LPCM formats.  No reference
 * counterpart.  The noise of a sample is a hash of (seed, port, index) -- one fmix per sample, two 64-bit multiplies, both 32-bit words
 * used -- so the bytes of a file do not depend on the window, the slicing, the sharding or the launch shape.  Product and adds of the
 * quantiser are __dmul_rn / __dadd_rn (dither.h): never contracted, the bits of the numpy restatement.  Loads, packing and the word-sized
 * non-temporal stores are those of the plain kernels, which serve every call with dither off.
 * ---------------------------------------------------------------------------------------------- */
static_assert(GDG_DITHER_K == GDG_DIGEST_K && GDG_DITHER_M0 == GDG_DIGEST_M0 && GDG_DITHER_M1 == GDG_DIGEST_M1, "the dither hashes with the digest's constants");

/* four consecutive samples of one port, the first at index `at`, into W whole words */
template <int FMT>
__device__ __forceinline__ void encode4_dither(const double (&r)[4], unsigned long long key, unsigned long long at, unsigned (&w)[fmt_width<FMT>::W]) {
    constexpr int W = fmt_width<FMT>::W;
#pragma unroll
    for (int k = 0; k < W; k++) w[k] = 0;
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const unsigned code = gdg_dither_code(FMT, r[s], key, at + (unsigned long long)s);
#pragma unroll
        for (int k = 0; k < W; k++) {
            int byte = s * W + k;
            w[byte >> 2] |= ((code >> (8 * k)) & 0xffu) << ((byte & 3) * 8);
        }
    }
}

/* wave_encode4_rows_kernel's sibling: blockIdx.y = row, whose port follows from the row number (uniform over the workgroup: the key is
 * made on the scalar unit); sample i of every row has index dz.first + i */
template <int FMT>
__global__ void __launch_bounds__(256)
wave_encode4_rows_dither_kernel(const double *__restrict__ in, size_t row_stride, size_t groups_per_row, unsigned *__restrict__ words, gdg_dither_rows dz) {
    constexpr int W = fmt_width<FMT>::W;
    const v2d *row = reinterpret_cast<const v2d *>(in + (size_t)blockIdx.y * row_stride);
    unsigned *dst = words + (size_t)blockIdx.y * groups_per_row * W;
    const unsigned long long key = gdg_dither_key(dz.seed, gdg_dither_row_port(dz.port_base, dz.n_chain, blockIdx.y));
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups_per_row; g += (size_t)gridDim.x * 256) {
        v2d a = __builtin_nontemporal_load(row + 2 * g), b = __builtin_nontemporal_load(row + 2 * g + 1);
        const double r[4] = { a.x, a.y, b.x, b.y };
        unsigned w[W];
        encode4_dither<FMT>(r, key, dz.first + 4ull * g, w);
#pragma unroll
        for (int k = 0; k < W; k++) __builtin_nontemporal_store(w[k], dst + g * W + k);
    }
}

/* finish_master_kernel's sibling: the same loads and the same adds in the same order; SUMS keeps the float64 sums for the meters and the
 * report BEFORE the dither; the left side is port 0xfffffffd, the right 0xfffffffe, the piece's first sample has index `first` */
template <int FMT, bool SUMS>
__global__ void __launch_bounds__(256)
finish_master_dither_kernel(const double *__restrict__ slab, size_t stride, int G, int has_aux, size_t groups, unsigned *__restrict__ words_left,
                            unsigned *__restrict__ words_right, double *__restrict__ sums, size_t sums_stride, unsigned long long seed,
                            unsigned long long first) {
    constexpr int W = fmt_width<FMT>::W;
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= groups) return;
    const size_t rs = stride / 2;                                  /* v2d per row */
    const v2d *col = reinterpret_cast<const v2d *>(slab) + 2 * g;
    v2d xa = { 0.0, 0.0 }, xb = { 0.0, 0.0 };
    if (has_aux) { const v2d *q = col + (size_t)(2 * G) * rs; xa = __builtin_nontemporal_load(q); xb = __builtin_nontemporal_load(q + 1); }
#pragma unroll
    for (int side = 0; side < 2; side++) {
        const v2d *p = col + (size_t)(side * G) * rs;
        v2d a = __builtin_nontemporal_load(p), b = __builtin_nontemporal_load(p + 1);
#pragma unroll 4
        for (int k = 1; k < G; k++) {
            p += rs;
            a += __builtin_nontemporal_load(p);
            b += __builtin_nontemporal_load(p + 1);
        }
        if (has_aux) { a += xa; b += xb; }
        if (SUMS) {
            v2d *out = reinterpret_cast<v2d *>(sums + (size_t)side * sums_stride) + 2 * g;
            out[0] = a;
            out[1] = b;
        }
        unsigned *words = side ? words_right : words_left;
        if (!words) continue;
        const unsigned long long key = gdg_dither_key(seed, side ? GDG_DITHER_PORT_MASTER_RIGHT : GDG_DITHER_PORT_MASTER_LEFT);
        const double r[4] = { a.x, a.y, b.x, b.y };
        unsigned w[W];
        encode4_dither<FMT>(r, key, first + 4ull * g, w);
#pragma unroll
        for (int k = 0; k < W; k++) __builtin_nontemporal_store(w[k], words + g * W + k);
    }
}

/* the stand-alone mono form: wave_encode4_kernel's sibling for the aligned bulk ... */
template <int FMT>
__global__ void __launch_bounds__(256)
wave_encode4_dither_kernel(const v2d *__restrict__ in, size_t groups, unsigned *__restrict__ words, unsigned long long key, unsigned long long first) {
    constexpr int W = fmt_width<FMT>::W;
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (size_t)gridDim.x * 256) {
        v2d a = __builtin_nontemporal_load(in + 2 * g), b = __builtin_nontemporal_load(in + 2 * g + 1);
        const double r[4] = { a.x, a.y, b.x, b.y };
        unsigned w[W];
        encode4_dither<FMT>(r, key, first + 4ull * g, w);
#pragma unroll
        for (int k = 0; k < W; k++) __builtin_nontemporal_store(w[k], words + g * W + k);
    }
}

/* ... and one sample per thread, byte stores: the n % 4 samples behind the bulk, or everything when a buffer is not aligned for it */
template <int FMT>
__global__ void __launch_bounds__(256)
wave_encode_dither_tail_kernel(const double *__restrict__ in, size_t n, unsigned char *__restrict__ data, unsigned long long key, unsigned long long first) {
    constexpr int W = fmt_width<FMT>::W;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const unsigned code = gdg_dither_code(FMT, in[i], key, first + (unsigned long long)i);
#pragma unroll
        for (int k = 0; k < W; k++) data[i * W + k] = (unsigned char)((code >> (8 * k)) & 0xffu);
    }
}

/* ------------------------------------------------------------------------------------------------
 * The trimmed encoders (trim.h; include/gdg.h, gdg_batch_set_trim): a gain per output port in front of the encoder.  No reference
 * counterpart.  y = x * g is ONE __dmul_rn -- rounded before the encoder's scale sees it, never contracted with it -- and then the plain
 * encoder's code (DITHER false: all six formats) or the dithered one's (DITHER true: the four LPCM formats) of y.  Siblings of the four
 * encode paths and of the stand-alone form: the same 16-byte non-temporal loads, packing and word-sized non-temporal stores; the plain
 * and the dithered kernels serve every call with the trim off.  A row's gain is uniform over its workgroup: read once
 * from a small device array through the scalar unit (the rows kernel) or a kernel argument (the finish and the stand-alone form).  IEEE64
 * has no code: the product's 8 bytes are the sample's (the plain path copies the rows; here a kernel has to touch them).
 * One FP64 multiply per sample beside 8 bytes read and 1 .. 8 written: no atomics, no LDS, no scratch.
 * ---------------------------------------------------------------------------------------------- */
template <int FMT, bool DITHER>
__device__ __forceinline__ unsigned trim_code(double y, unsigned long long key, unsigned long long at) {
    if (DITHER) return gdg_dither_code(FMT, y, key, at);
    return encode_code<FMT>(y);
}

/* four consecutive samples of one port times its gain, the first at index `at`, into W whole words */
template <int FMT, bool DITHER>
__device__ __forceinline__ void encode4_trim(const double (&r)[4], double g, unsigned long long key, unsigned long long at, unsigned (&w)[fmt_width<FMT>::W]) {
    constexpr int W = fmt_width<FMT>::W;
#pragma unroll
    for (int k = 0; k < W; k++) w[k] = 0;
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const unsigned code = trim_code<FMT, DITHER>(gdg_trim_apply(r[s], g), key, at + (unsigned long long)s);
#pragma unroll
        for (int k = 0; k < W; k++) {
            int byte = s * W + k;
            w[byte >> 2] |= ((code >> (8 * k)) & 0xffu) << ((byte & 3) * 8);
        }
    }
}

/* a group's four samples from their two 16-byte halves, trimmed, encoded and stored: `words` is the row's (or the side's) first word */
template <int FMT, bool DITHER>
__device__ __forceinline__ void store4_trim(v2d a, v2d b, double g, unsigned long long key, unsigned long long at, unsigned *words, size_t group) {
    if (FMT == GDG_FMT_IEEE64) {
        const v2d ya = { gdg_trim_apply(a.x, g), gdg_trim_apply(a.y, g) }, yb = { gdg_trim_apply(b.x, g), gdg_trim_apply(b.y, g) };
        if (((uintptr_t)words & 15) == 0) {                            /* uniform: 16-byte stores where the row allows them, the 8-byte rule otherwise */
            v2d *out = reinterpret_cast<v2d *>(words) + 2 * group;
            __builtin_nontemporal_store(ya, out);
            __builtin_nontemporal_store(yb, out + 1);
        } else {
            double *out = reinterpret_cast<double *>(words) + 4 * group;
            __builtin_nontemporal_store(ya.x, out);
            __builtin_nontemporal_store(ya.y, out + 1);
            __builtin_nontemporal_store(yb.x, out + 2);
            __builtin_nontemporal_store(yb.y, out + 3);
        }
    } else {
        constexpr int W = fmt_width<FMT>::W;
        const double r[4] = { a.x, a.y, b.x, b.y };
        unsigned w[W];
        encode4_trim<FMT, DITHER>(r, g, key, at, w);
#pragma unroll
        for (int k = 0; k < W; k++) __builtin_nontemporal_store(w[k], words + group * W + k);
    }
}

/* words of 32 bits per group of four samples */
template <int FMT> struct trim_group_words { static const int N = FMT == GDG_FMT_IEEE64 ? 8 : fmt_width<FMT>::W; };

/* wave_encode4_rows_kernel's and wave_encode4_rows_dither_kernel's sibling: blockIdx.y = row, gains[row] its gain */
template <int FMT, bool DITHER>
__global__ void __launch_bounds__(256)
wave_encode4_rows_trim_kernel(const double *__restrict__ in, size_t row_stride, size_t groups_per_row, unsigned *__restrict__ words,
                              const double *__restrict__ gains, gdg_dither_rows dz) {
    const v2d *row = reinterpret_cast<const v2d *>(in + (size_t)blockIdx.y * row_stride);
    unsigned *dst = words + (size_t)blockIdx.y * groups_per_row * trim_group_words<FMT>::N;
    const double g = gains[blockIdx.y];
    const unsigned long long key = DITHER ? gdg_dither_key(dz.seed, gdg_dither_row_port(dz.port_base, dz.n_chain, blockIdx.y)) : 0ull;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < groups_per_row; i += (size_t)gridDim.x * 256) {
        v2d a = __builtin_nontemporal_load(row + 2 * i), b = __builtin_nontemporal_load(row + 2 * i + 1);
        store4_trim<FMT, DITHER>(a, b, g, key, dz.first + 4ull * i, dst, i);
    }
}

/* finish_master_kernel's and finish_master_dither_kernel's sibling: the same loads and the same adds in the same order; SUMS keeps the
 * float64 sums for the meters and the records BEFORE the trim; the left side is encoded times gain_left, the right times gain_right */
template <int FMT, bool SUMS, bool DITHER>
__global__ void __launch_bounds__(256)
finish_master_trim_kernel(const double *__restrict__ slab, size_t stride, int G, int has_aux, size_t groups, unsigned *__restrict__ words_left,
                          unsigned *__restrict__ words_right, double *__restrict__ sums, size_t sums_stride, double gain_left, double gain_right,
                          unsigned long long seed, unsigned long long first) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= groups) return;
    const size_t rs = stride / 2;                                  /* v2d per row */
    const v2d *col = reinterpret_cast<const v2d *>(slab) + 2 * g;
    v2d xa = { 0.0, 0.0 }, xb = { 0.0, 0.0 };
    if (has_aux) { const v2d *q = col + (size_t)(2 * G) * rs; xa = __builtin_nontemporal_load(q); xb = __builtin_nontemporal_load(q + 1); }
#pragma unroll
    for (int side = 0; side < 2; side++) {
        const v2d *p = col + (size_t)(side * G) * rs;
        v2d a = __builtin_nontemporal_load(p), b = __builtin_nontemporal_load(p + 1);
#pragma unroll 4
        for (int k = 1; k < G; k++) {
            p += rs;
            a += __builtin_nontemporal_load(p);
            b += __builtin_nontemporal_load(p + 1);
        }
        if (has_aux) { a += xa; b += xb; }
        if (SUMS) {
            v2d *out = reinterpret_cast<v2d *>(sums + (size_t)side * sums_stride) + 2 * g;
            out[0] = a;
            out[1] = b;
        }
        unsigned *words = side ? words_right : words_left;
        if (!words) continue;
        const unsigned long long key = DITHER ? gdg_dither_key(seed, side ? GDG_DITHER_PORT_MASTER_RIGHT : GDG_DITHER_PORT_MASTER_LEFT) : 0ull;
        store4_trim<FMT, DITHER>(a, b, side ? gain_right : gain_left, key, first + 4ull * g, words, g);
    }
}

/* the stand-alone mono form: wave_encode4_kernel's and wave_encode4_dither_kernel's sibling for the aligned bulk ... */
template <int FMT, bool DITHER>
__global__ void __launch_bounds__(256)
wave_encode4_trim_kernel(const v2d *__restrict__ in, size_t groups, unsigned *__restrict__ words, double g, unsigned long long key, unsigned long long first) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < groups; i += (size_t)gridDim.x * 256) {
        v2d a = __builtin_nontemporal_load(in + 2 * i), b = __builtin_nontemporal_load(in + 2 * i + 1);
        store4_trim<FMT, DITHER>(a, b, g, key, first + 4ull * i, words, i);
    }
}

/* ... and one sample per thread, 8-byte loads and byte stores: the n % 4 samples behind the bulk, or everything when a buffer is not aligned for it */
template <int FMT, bool DITHER>
__global__ void __launch_bounds__(256)
wave_encode_trim_tail_kernel(const double *__restrict__ in, size_t n, unsigned char *__restrict__ data, double g, unsigned long long key, unsigned long long first) {
    constexpr int BYTES = FMT == GDG_FMT_IEEE64 ? 8 : fmt_width<FMT>::W;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const double y = gdg_trim_apply(in[i], g);
        unsigned long long bits;
        if (FMT == GDG_FMT_IEEE64) bits = (unsigned long long)__double_as_longlong(y);
        else bits = trim_code<FMT, DITHER>(y, key, first + (unsigned long long)i);
#pragma unroll
        for (int k = 0; k < BYTES; k++) data[i * BYTES + k] = (unsigned char)((bits >> (8 * k)) & 0xffu);
    }
}

/* ------------------------------------------------------------------------------------------------
 * The encode launchers: one per form -- rows of a window, the master finish, stand-alone mono -- for the three generations of kernels
 * above.  A gdg_encode_mode says what the launch does beyond the plain encoder; GDG_DISPATCH_ENCODE turns it and the format into the
 * constants <FMT, TRIM, DITHER>, and each launch template picks the kernel of that generation: the trimmed one (plain or dithered) when
 * TRIM, else the dithered one when DITHER, else the plain one.  The kernels' texts are kept apart on purpose: folded into one template
 * the untrimmed instantiations compiled to other instruction streams than these (profiles/encode_one_path.txt).
 * ---------------------------------------------------------------------------------------------- */
/* STMT once with FMT, TRIM and DITHER constants, as the mode M has them: all six formats undithered, the four LPCM formats dithered (the
 * callers send the IEEE formats here with dither off: gdg_dither_applies) */
#define GDG_DISPATCH_ENCODE(F, M, STMT)                                                                                 \
    if ((M).dither) {                                                                                                   \
        constexpr bool DITHER = true;                                                                                   \
        if ((M).trim) { constexpr bool TRIM = true; GDG_DISPATCH_LPCM(F, STMT) }                                        \
        else { constexpr bool TRIM = false; GDG_DISPATCH_LPCM(F, STMT) }                                                \
    } else {                                                                                                            \
        constexpr bool DITHER = false;                                                                                  \
        if ((M).trim) { constexpr bool TRIM = true; GDG_DISPATCH_FMT(F, STMT) }                                         \
        else { constexpr bool TRIM = false; GDG_DISPATCH_FMT(F, STMT) }                                                 \
    }

template <int FMT, bool TRIM, bool DITHER>
static hipError_t launch_encode_rows(const double *d_in, size_t row_stride, size_t row_len, unsigned n_rows, void *d_bytes, const gdg_encode_mode &m, hipStream_t s) {
    if constexpr (FMT == GDG_FMT_IEEE64 && !TRIM)                  /* wave.go:694-709: the sample's bytes, no clipping -- a copy */
        return hipMemcpy2DAsync(d_bytes, row_len * sizeof(double), d_in, row_stride * sizeof(double), row_len * sizeof(double), n_rows, hipMemcpyDeviceToDevice, s);
    else {
        const size_t groups = row_len / 4;
        const dim3 grid((unsigned)((groups + 255) / 256), n_rows);
        unsigned *words = static_cast<unsigned *>(d_bytes);
        if constexpr (TRIM) wave_encode4_rows_trim_kernel<FMT, DITHER><<<grid, dim3(256), 0, s>>>(d_in, row_stride, groups, words, m.d_gains, m.dz);
        else if constexpr (DITHER) wave_encode4_rows_dither_kernel<FMT><<<grid, dim3(256), 0, s>>>(d_in, row_stride, groups, words, m.dz);
        else wave_encode4_rows_kernel<FMT><<<grid, dim3(256), 0, s>>>(d_in, row_stride, groups, words);
        return hipGetLastError();
    }
}

hipError_t gdg_launch_wave_encode_rows(int fmt, const double *d_in, size_t row_stride, size_t row_len, unsigned n_rows, void *d_bytes,
                                       const gdg_encode_mode &m, hipStream_t s) {
    if (n_rows == 0 || row_len == 0) return hipSuccess;
    if ((m.trim && (!m.d_gains || ((uintptr_t)m.d_gains & 7))) || (row_len & 3) || (row_stride & 1) || ((uintptr_t)d_in & 15) ||
        ((uintptr_t)d_bytes & (m.trim && fmt == GDG_FMT_IEEE64 ? 7 : 3)))      /* the trimmed IEEE64 rows are written 8 bytes at a time */
        return hipErrorInvalidValue;
    GDG_DISPATCH_ENCODE(fmt, m, return (launch_encode_rows<FMT, TRIM, DITHER>(d_in, row_stride, row_len, n_rows, d_bytes, m, s)));
}

template <int FMT, bool SUMS, bool TRIM, bool DITHER>
static void launch_finish_master_sums(const double *d_slab, size_t stride, int G, int has_aux, size_t groups, unsigned *wl, unsigned *wr, double *d_sums,
                                      size_t sums_stride, const gdg_encode_mode &m, hipStream_t s) {
    const unsigned grid = (unsigned)((groups + 255) / 256);
    if constexpr (TRIM)
        finish_master_trim_kernel<FMT, SUMS, DITHER><<<grid, 256, 0, s>>>(d_slab, stride, G, has_aux, groups, wl, wr, d_sums, sums_stride, m.gain[0], m.gain[1], m.dz.seed, m.dz.first);
    else if constexpr (DITHER)
        finish_master_dither_kernel<FMT, SUMS><<<grid, 256, 0, s>>>(d_slab, stride, G, has_aux, groups, wl, wr, d_sums, sums_stride, m.dz.seed, m.dz.first);
    else
        finish_master_kernel<FMT, SUMS><<<grid, 256, 0, s>>>(d_slab, stride, G, has_aux, groups, wl, wr, d_sums, sums_stride);
}

template <int FMT, bool TRIM, bool DITHER>
static hipError_t launch_finish_master(const double *d_slab, size_t stride, int G, int has_aux, size_t n, void *d_left, void *d_right, double *d_sums,
                                       size_t sums_stride, const gdg_encode_mode &m, hipStream_t s) {
    unsigned *wl = static_cast<unsigned *>(d_left), *wr = static_cast<unsigned *>(d_right);
    if (d_sums) launch_finish_master_sums<FMT, true, TRIM, DITHER>(d_slab, stride, G, has_aux, n / 4, wl, wr, d_sums, sums_stride, m, s);
    else launch_finish_master_sums<FMT, false, TRIM, DITHER>(d_slab, stride, G, has_aux, n / 4, wl, wr, nullptr, 0, m, s);
    return hipGetLastError();
}

hipError_t gdg_launch_finish_master(int fmt, const double *d_slab, size_t stride, int n_shards, int has_aux, size_t n, void *d_left_bytes,
                                    void *d_right_bytes, double *d_sums, size_t sums_stride, const gdg_encode_mode &m, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (n_shards < 1 || (n & 3) || n > stride || (stride & 1) || (sums_stride & 1) || (d_sums && n > sums_stride) || ((uintptr_t)d_slab & 15) ||
        ((uintptr_t)d_left_bytes & 15) || ((uintptr_t)d_right_bytes & 15) || ((uintptr_t)d_sums & 15))
        return hipErrorInvalidValue;
    GDG_DISPATCH_ENCODE(fmt, m, return (launch_finish_master<FMT, TRIM, DITHER>(d_slab, stride, n_shards, has_aux, n, d_left_bytes, d_right_bytes, d_sums, sums_stride, m, s)));
}

template <int FMT, bool TRIM, bool DITHER>
static hipError_t launch_encode(const double *d_in, size_t per, unsigned channels, unsigned char *p, const gdg_encode_mode &m, hipStream_t s) {
    constexpr size_t BYTES = FMT == GDG_FMT_IEEE64 ? 8 : fmt_width<FMT>::W;     /* per sample */
    const unsigned long long key = DITHER ? gdg_dither_key(m.dz.seed, m.dz.port_base) : 0ull, first = m.dz.first;
    size_t n = per * channels, done = 0;
    /* the untrimmed IEEE64 bytes are the samples: the one-sample kernel copies them, whatever the alignment */
    if ((TRIM || FMT != GDG_FMT_IEEE64) && channels == 1 && n >= 4 && ((uintptr_t)p & (FMT == GDG_FMT_IEEE64 ? 7 : 3)) == 0 && ((uintptr_t)d_in & 15) == 0) {
        const size_t groups = n / 4;
        const unsigned grid = (unsigned)((groups + 255) / 256);
        const v2d *in = reinterpret_cast<const v2d *>(d_in);
        unsigned *words = reinterpret_cast<unsigned *>(p);
        if constexpr (TRIM) wave_encode4_trim_kernel<FMT, DITHER><<<grid, 256, 0, s>>>(in, groups, words, m.gain[0], key, first);
        else if constexpr (DITHER) wave_encode4_dither_kernel<FMT><<<grid, 256, 0, s>>>(in, groups, words, key, first);
        else wave_encode4_kernel<FMT><<<grid, 256, 0, s>>>(in, groups, words);
        done = groups * 4;
    }
    if (done < n) {         /* tail and unaligned buffers, and the plain encoder's multi-channel files: one sample per thread */
        if constexpr (TRIM) wave_encode_trim_tail_kernel<FMT, DITHER><<<grid_for(n - done), 256, 0, s>>>(d_in + done, n - done, p + done * BYTES, m.gain[0], key, first + done);
        else if constexpr (DITHER) wave_encode_dither_tail_kernel<FMT><<<grid_for(n - done), 256, 0, s>>>(d_in + done, n - done, p + done * BYTES, key, first + done);
        else if (channels == 1) wave_encode_kernel<FMT><<<grid_for(n - done), 256, 0, s>>>(d_in + done, n - done, p + done * BYTES, 1, n - done);
        else wave_encode_kernel<FMT><<<grid_for(n), 256, 0, s>>>(d_in, n, p, channels, per);
    }
    return hipGetLastError();
}

/* trimmed or dithered: mono, any 8-byte alignment of d_in and any byte alignment of d_bytes */
hipError_t gdg_launch_wave_encode(int fmt, const double *d_in, size_t per, unsigned channels, void *d_bytes, const gdg_encode_mode &m, hipStream_t s) {
    if (per * channels == 0) return hipSuccess;
    if ((m.trim || m.dither) && (channels != 1 || ((uintptr_t)d_in & 7))) return hipErrorInvalidValue;
    GDG_DISPATCH_ENCODE(fmt, m, return (launch_encode<FMT, TRIM, DITHER>(d_in, per, channels, static_cast<unsigned char *>(d_bytes), m, s)));
}

/* ------------------------------------------------------------------------------------------------
 * The render report (include/gdg.h, gdg_block_stats): peak, sum of squares and three counts per block of a row.  No reference
 * counterpart.  One workgroup of 256 threads per (block, row): blockIdx.x = block, blockIdx.y = row.
 *
 * The order of every operation is a function of the block's length L alone:
 *   thread t walks the sample pairs p = t, t + 256, t + 512 ... (2 p < L), the samples 2 p and 2 p + 1 of each one after the other, into
 *   ONE running sum and one running (peak, index) -- indices ascend, so "strictly greater" keeps the first;
 *   the 64 lanes of a wave meet in the fixed tree lane i <- lane i + 32, + 16 .. + 1; the four wave results through LDS, added 0, 1, 2, 3.
 * Nothing depends on the row, the grid, where the block lies or who arrives first, and the square and the adds are __dmul_rn / __dadd_rn
 * (never contracted): the same samples give the same 64 bits wherever they sit and however this file is compiled.  VEC reads a pair with
 * one 16-byte load where the launcher has seen that every block starts 16-byte aligned and `block` is even; the values and their order
 * are the scalar path's.  A pair's second sample is read only when it lies inside the block: nothing outside [row, row + samples).
 * ---------------------------------------------------------------------------------------------- */
#define STATS_T 256
struct StatsAcc { double peak, ssq; unsigned idx, clipped, full, nonfin; };
__device__ __forceinline__ void stats_take(StatsAcc &a, double x, unsigned i) {
    const double m = fabs(x);
    if (m <= 1.7976931348623157e308) {                  /* finite: false for NaN and for +-inf */
        if (m > a.peak) { a.peak = m; a.idx = i; }
        a.ssq = __dadd_rn(a.ssq, __dmul_rn(x, x));
        a.clipped += m > 1.0 ? 1u : 0u;
        a.full += m >= 1.0 ? 1u : 0u;
    } else a.nonfin++;
}
/* the pair (peak, index) in the order "larger peak, then lower index"; sums as (mine + theirs) */
__device__ __forceinline__ void stats_join(StatsAcc &a, double peak, unsigned idx, double ssq, unsigned clipped, unsigned full, unsigned nonfin) {
    if (peak > a.peak || (peak == a.peak && idx < a.idx)) { a.peak = peak; a.idx = idx; }
    a.ssq = __dadd_rn(a.ssq, ssq);
    a.clipped += clipped;
    a.full += full;
    a.nonfin += nonfin;
}

template <bool VEC>
__global__ void __launch_bounds__(STATS_T)
block_stats_kernel(const double *__restrict__ rows, size_t row_stride, size_t samples, unsigned block, unsigned row0, unsigned blocks_per_row,
                   gdg_block_stats *__restrict__ records) {
    __shared__ double s_peak[STATS_T / 64], s_ssq[STATS_T / 64];
    __shared__ unsigned s_idx[STATS_T / 64], s_cnt[STATS_T / 64][3];
    const unsigned tid = threadIdx.x, lane = tid & 63u, row = row0 + blockIdx.y;
    const size_t first = (size_t)blockIdx.x * block;
    const unsigned L = (unsigned)(samples - first < (size_t)block ? samples - first : (size_t)block);
    const double *x = rows + (size_t)row * row_stride + first;
    StatsAcc a = { 0.0, 0.0, 0u, 0u, 0u, 0u };
    /* four pairs per round, their loads in flight together; the sums follow in the pairs' order */
    for (unsigned p0 = tid; 2u * p0 < L; p0 += 4u * STATS_T) {
        double v[4][2];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned i = 2u * (p0 + (unsigned)k * STATS_T);
            v[k][0] = v[k][1] = 0.0;
            if (VEC && i + 1u < L) {
                const v2d q = *reinterpret_cast<const v2d *>(x + i);
                v[k][0] = q.x;
                v[k][1] = q.y;
            } else {
                if (i < L) v[k][0] = x[i];
                if (i + 1u < L) v[k][1] = x[i + 1u];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned i = 2u * (p0 + (unsigned)k * STATS_T);
            if (i < L) stats_take(a, v[k][0], i);
            if (i + 1u < L) stats_take(a, v[k][1], i + 1u);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        stats_join(a, __shfl_down(a.peak, o), __shfl_down(a.idx, o), __shfl_down(a.ssq, o), __shfl_down(a.clipped, o), __shfl_down(a.full, o),
                   __shfl_down(a.nonfin, o));
    if (lane == 0) {
        const unsigned w = tid >> 6;
        s_peak[w] = a.peak; s_ssq[w] = a.ssq; s_idx[w] = a.idx;
        s_cnt[w][0] = a.clipped; s_cnt[w][1] = a.full; s_cnt[w][2] = a.nonfin;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < STATS_T / 64; w++) stats_join(a, s_peak[w], s_idx[w], s_ssq[w], s_cnt[w][0], s_cnt[w][1], s_cnt[w][2]);
        gdg_block_stats *r = records + (size_t)row * blocks_per_row + blockIdx.x;
        r->peak = a.peak;
        r->sum_sq = a.ssq;
        r->peak_index = a.idx;
        r->clipped = a.clipped;
        r->full_scale = a.full;
        r->nonfinite = a.nonfin;
    }
}

hipError_t gdg_launch_block_stats(const double *d_rows, size_t row_stride, unsigned n_rows, size_t samples, unsigned block, void *d_out, hipStream_t s) {
    gdg_block_stats *d_records = static_cast<gdg_block_stats *>(d_out);
    if (n_rows == 0 || samples == 0) return hipSuccess;
    if (block == 0) return hipErrorInvalidValue;
    const size_t blocks = (samples + block - 1) / block;
    if (row_stride < samples || blocks > 0x7fffffffu || ((uintptr_t)d_rows & 7) || ((uintptr_t)d_records & 7)) return hipErrorInvalidValue;
    const bool vec = !((uintptr_t)d_rows & 15) && !(row_stride & 1) && !(block & 1);
    for (unsigned r0 = 0; r0 < n_rows; r0 += 65535u) {                      /* gridDim.y holds 65535 rows */
        const dim3 grid((unsigned)blocks, n_rows - r0 < 65535u ? n_rows - r0 : 65535u);
        if (vec) block_stats_kernel<true><<<grid, STATS_T, 0, s>>>(d_rows, row_stride, samples, block, r0, (unsigned)blocks, d_records);
        else block_stats_kernel<false><<<grid, STATS_T, 0, s>>>(d_rows, row_stride, samples, block, r0, (unsigned)blocks, d_records);
    }
    return hipGetLastError();
}

#include "true_peak_kernels.h"      /* the render report's true-peak record: the same rows, the same load rule */
#include "blend_kernels.h"          /* the blend outputs: weighted sums of the window's chain rows, in front of the encoders and the records */
#include "fit_kernels.h"            /* the blend fit's records: inner products of the window's rows in block_stats_kernel's order of sums */
#include "deliver_kernels.h"        /* the delivery at a half or a quarter of the session rate: the window's rows decimated in front of the encoders */
#include "deliver_ratio_kernels.h"  /* ... and the ratio stage behind it: the intermediate rows resampled by L / M, polyphase */
#include "delivered_kernels.h"      /* the records of the delivered rows: blocks of any length, a true peak that is seamless across them */

/* resample.Time over a span of a file (the streamed batch run): blockIdx.y = input. Output samples [out_first, out_first + count) from
 * the source frames [src_first, src_first + src_count) at `src`; n = the FILE's frames (the j < n bound).  x, floor(x) and x - j are
 * formed from the absolute 64-bit i and j in the operation order of resample_time_kernel, so every sample has the whole-file kernel's
 * bits (both kernels are compiled without contraction).  The host sizes the span so that every j in [0, n) a sample reads lies inside
 * it (gdg_batch_stream_span); the bounds test on the span itself is there so that a wrong span can never read outside the buffer.
 * The last workgroup of an input also copies the span's last `keep` frames to `carry`: the frames the next slice looks back at. */
__global__ void __launch_bounds__(256)
resample_span_kernel(const gdg_resample_span *__restrict__ spans) {
    const gdg_resample_span r = spans[blockIdx.y];
    for (unsigned k = blockIdx.x * 256 + threadIdx.x; k < r.count; k += gridDim.x * 256) {
        const long long i = r.out_first + (long long)k;
        double x = (double)i * r.dx;
        long long idx = (long long)floor(x);
        double sum = 0.0;
#pragma unroll
        for (long long j = idx - 2; j < idx + 4; j++) {
            if (j >= 0 && j < r.n) {
                double diff = x - (double)j;
                const long long at = j - r.src_first;
                const double v = (at >= 0 && at < (long long)r.src_count) ? r.src[at] : 0.0;
                sum += v * lanczos_kernel(diff, 3.0);
            }
        }
        r.dst[k] = sum;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x < r.keep) r.carry[threadIdx.x] = r.src[r.src_count - r.keep + threadIdx.x];
}

hipError_t gdg_launch_resample_spans(const gdg_resample_span *d_spans, int n_spans, unsigned max_count, hipStream_t s) {
    if (n_spans <= 0) return hipSuccess;
    unsigned tiles = (max_count + 255) / 256;
    if (tiles > 256) tiles = 256;
    if (tiles == 0) tiles = 1;
    resample_span_kernel<<<dim3(tiles, (unsigned)n_spans), dim3(256), 0, s>>>(d_spans);
    return hipGetLastError();
}

/* resample_span_kernel with a fan: the six weights and the sum are formed once per output sample -- the same operations in the same order,
 * so every row gets the bits the single-row kernel gives -- and stored to every row of the fan, a row at a time across the lanes.  The
 * carry is the root's, kept once. */
__global__ void __launch_bounds__(256)
resample_fans_kernel(const gdg_resample_fan *__restrict__ fans, double *const *__restrict__ table) {
    const gdg_resample_span r = fans[blockIdx.y].span;
    double *const *rows = table + fans[blockIdx.y].dst_first;
    const unsigned n_dst = fans[blockIdx.y].n_dst;
    for (unsigned k = blockIdx.x * 256 + threadIdx.x; k < r.count; k += gridDim.x * 256) {
        const long long i = r.out_first + (long long)k;
        double x = (double)i * r.dx;
        long long idx = (long long)floor(x);
        double sum = 0.0;
#pragma unroll
        for (long long j = idx - 2; j < idx + 4; j++) {
            if (j >= 0 && j < r.n) {
                double diff = x - (double)j;
                const long long at = j - r.src_first;
                const double v = (at >= 0 && at < (long long)r.src_count) ? r.src[at] : 0.0;
                sum += v * lanczos_kernel(diff, 3.0);
            }
        }
        for (unsigned d = 0; d < n_dst; d++) rows[d][k] = sum;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x < r.keep) r.carry[threadIdx.x] = r.src[r.src_count - r.keep + threadIdx.x];
}

hipError_t gdg_launch_resample_fans(const gdg_resample_fan *d_fans, double *const *d_table, int n_fans, unsigned max_count, hipStream_t s) {
    if (n_fans <= 0) return hipSuccess;
    unsigned tiles = (max_count + 255) / 256;
    if (tiles > 256) tiles = 256;
    if (tiles == 0) tiles = 1;
    resample_fans_kernel<<<dim3(tiles, (unsigned)n_fans), dim3(256), 0, s>>>(d_fans, d_table);
    return hipGetLastError();
}

hipError_t gdg_launch_resample_time(const double *d_in, int n, double dx, double *d_out, int n_out, hipStream_t s) {
    if (n_out <= 0) return hipSuccess;
    resample_time_kernel<<<grid_for((size_t)n_out), 256, 0, s>>>(d_in, n, dx, d_out, n_out);
    return hipGetLastError();
}
