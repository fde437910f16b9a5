/*
 * gdg_internal.h -- structures shared by the host side (api_*.cpp, ctx.h) and the HIP kernels.
 * Not part of the ABI.
 */
#ifndef GDG_INTERNAL_H
#define GDG_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "spectrum_bands.h"
#include "align_map.h"
#include "true_peak_taps.h"

#define GDG_MAX_FRAMES 8192          /* controller/controller.go:36 BLOCK_SIZE; one frame must fit the LDS */
#define GDG_MIN_FIR_FRAMES 64

/* ------------------------------------------------------------------------------------------------
 * FIR (power amp) -- uniformly partitioned overlap-save convolution, partition = frame.
 *
 * Per FIR unit and channel, in HBM:
 *   prev  [P]            last frame's input (overlap-save history)
 *   fdl   [K][P] cplx    frequency-domain delay line, slot s holds the packed half spectrum
 *                        (P complex128; bin 0 carries (Re X[0], Re X[P])) of [x_{t-1} | x_t]
 *   H     [K][P] cplx    packed half spectra of the IR partitions, pre-scaled by 1/(2P)
 *   Y     [P]    cplx    accumulated product spectrum (scratch between MAC and inverse)
 *   pos   int[4]         [0] frame counter; slot of the current frame = pos % R.  [1], [2]: the frame counter and the epoch the sums
 *                        made ahead were made for (fir_ahead_kernel; epoch 0 = none)
 *   acc   [T][P] cplx    sums made ahead (fir_ahead_kernel): acc[j] = the terms k = K - 1 .. j + 1 of frame pos[1] + j
 * ---------------------------------------------------------------------------------------------- */
/* A plan's descriptors hold absolute pointers; those into the caller's buffers are flagged, and every launch carries the distance
 * (in samples) from the buffers the plan was built on to the ones of this call -- walking through a file does not rebuild the plan. */
#define GDG_SRC_IS_INPUT 1
#define GDG_DST_IS_OUTPUT 2
#define GDG_DST_UNUSED 4             /* FIR unit whose output frame is consumed by a chained forward transform only (fir_inv_kernel, CHAIN) */
struct gdg_shift { long long in, out; };

struct gdg_fir_chan {
    const double *src;       /* current frame, `hop` samples */
    double *dst;             /* output frame, `hop` samples */
    double *prev;            /* [2][P]: the previous frame, ping-pong by frame parity */
    double2 *fdl;
    const double2 *H;
    double2 *Y;
    int *pos;
    double2 *acc;            /* [T][P] sums made ahead of the next T frames (per-frame calls, Shape FUSED_AHEAD); null elsewhere */
    int K;
    int R;                   /* slots of the delay-line ring: K, or K + W - 1 when the context runs windows of W blocks (time blocking) */
    int flags;               /* GDG_SRC_IS_INPUT / GDG_DST_IS_OUTPUT */
    int hop;                 /* samples per frame; == P for power-of-two frames, < P otherwise (the transform of
                              * [previous | current | zeros] still has 2P points, P = nextpow2(hop)) */
};

/* one forward transform job: [a | b | zeros] -> out.  IR spectra: a = one partition zero padded to P samples, b = NULL (zeros),
 * hop = 0.  Re-partitioning of a live delay line (frame size change): a, b = two consecutive frames of `hop` samples. */
struct gdg_fir_irjob {
    const double *a;
    double2 *out;            /* P complex */
    const double *b;
    int hop;                 /* 0: a holds P samples, b is not read */
    int pad;
};

/* one raw inverse transform job (frame size change): packed half spectrum Y of [first | second | zeros] -> the two frames of
 * `hop` samples, unclipped, scaled by `scale`; `first` may be NULL */
struct gdg_fir_rawjob {
    const double2 *Y;
    double *first, *second;
    int hop, pad;
};

/* process-wide launch-shape knobs of fir.hip / the tuner (their launchers have no context); set through gdg_ctx_set_option */
enum { GDG_KNOB_FFT_HALF_LDS = 0, GDG_KNOB_FWD_PER_CHANNEL, GDG_KNOB_WAVE_FFT, GDG_KNOB_MAC_VARIANT, GDG_KNOB_TUNER_PARTS, GDG_KNOB_COUNT };
int gdg_knob_get(int which);
void gdg_knob_set(int which, int value);

/* launchers implemented in fir.hip; all return hipError_t */
hipError_t gdg_fir_tables_create(int P, double2 **d_tw, double2 **d_tw2);
hipError_t gdg_launch_fir_fwd(int P, int hop, const gdg_fir_chan *d_chans, int n_chans, const double2 *d_tw, const double2 *d_tw2, gdg_shift shift, hipStream_t s);
/* k_lo: the partitions k = K - 1 .. k_lo are summed (descending: the order of every multiply-accumulate kernel).  0 = the whole sum;
 * 1 = everything but the newest partition, i.e. what can be computed BEFORE the frame exists (the premac of small shards, api_process.cpp) */
hipError_t gdg_launch_fir_mac(int P, const gdg_fir_chan *d_chans, int n_chans, int shared_spectra, hipStream_t s, int k_lo = 0, int lds_bytes = 0);
/* time blocking: a window of W (2, 4, 8 or 16) consecutive 8192-sample frames per channel; what = 0 forward transforms, 1 multiply-accumulate
 * (reads every spectrum once for the W frames), 2 inverse transforms, 3 history + frame counter.  chans[].src / dst: frame 0 of the
 * window, frame j at + j * 8192; chans[].Y holds W spectra; chans[].R >= K + W - 1. */
hipError_t gdg_launch_fir_window(int W, const gdg_fir_chan *d_chans, int n_chans, int shared_spectra, const double2 *d_tw, const double2 *d_tw2,
                                 int what, gdg_shift shift, hipStream_t s);
/* d_next_chans != NULL (P == 8192, frames of 8192): descriptor i is the power amp that follows chans[i] in the same channel's chain; its
 * forward transform (history + delay-line slot) is produced by this launch and gdg_launch_fir_fwd is NOT called for it */
/* time blocking with adjacent power amps: what = 2 of d_chans and what = 0 of d_next_chans in one launch (needs gdg_fir_window_chain_ok) */
int gdg_fir_window_chain_ok(int n_chans, int W);
hipError_t gdg_launch_fir_window_chain(int W, const gdg_fir_chan *d_chans, const gdg_fir_chan *d_next_chans, int n_chans, const double2 *d_tw,
                                       const double2 *d_tw2, gdg_shift shift, hipStream_t s);
/* Sums made ahead of several frames (fused = 5 / 6 below): the sums of frame t hold the terms k = K - 1 .. j + 1 for j = t - stamp; `epoch` is
 * the context's current one (a stamp of another epoch is never read), T the frames one pass serves (2 .. 4); `used` (may be null) counts the
 * workgroups -- channel frames -- that continued sums made ahead */
struct gdg_ahead { unsigned epoch; int T; unsigned long long *used; };
hipError_t gdg_launch_fir_inv(int P, const gdg_fir_chan *d_chans, int n_chans, const double2 *d_tw, const double2 *d_tw2, int fused, gdg_shift shift, hipStream_t s,
                              const gdg_fir_chan *d_next_chans = nullptr, hipEvent_t ev_begin = nullptr, hipEvent_t ev_end = nullptr,
                              gdg_ahead ahead = gdg_ahead{ 0u, 0, nullptr });
/* the pass ahead (P = 8192 only): for every step s < n_steps, the channels [first, first + n) of d_chans[s] get acc[j] = the terms
 * k = K - 1 .. j + 1 of frame pos + j, j = 0 .. min(T, K - 1) - 1, and the stamp (pos, epoch); shared_spectra as gdg_launch_fir_mac */
#define GDG_AHEAD_MAX_STEPS 4
struct gdg_ahead_steps { const gdg_fir_chan *chans[GDG_AHEAD_MAX_STEPS]; int n_steps; int first, n; int shared_mask; };
hipError_t gdg_launch_fir_ahead(int P, const gdg_ahead_steps &steps, gdg_ahead ahead, hipStream_t s);
hipError_t gdg_launch_fir_ir(int P, const gdg_fir_irjob *d_jobs, int n_jobs, double scale, const double2 *d_tw, const double2 *d_tw2, hipStream_t s);
hipError_t gdg_launch_fir_raw_inv(int P, const gdg_fir_rawjob *d_jobs, int n_jobs, double scale, const double2 *d_tw, const double2 *d_tw2, hipStream_t s);

/* ------------------------------------------------------------------------------------------------
 * Segments -- the per-sample units between FIR units, fused into one launch (seg.hip).
 * One workgroup per channel; the frame lives in LDS; per-unit state lives in HBM:
 *   ds   [GDG_DS_LEN] doubles   small state (envelopes, capacitor voltages, LFO phase ...)
 *   is   [GDG_IS_LEN] ints      FSM state, ring write positions
 *   hist [..] doubles           input-history / all-pass rings (length depends on the sample rate)
 * dp / jp carry constants derived on the host from the resolved parameters in exactly the
 * reference's arithmetic (e.g. 10^(dB/20), 1 - exp(-2 pi f / sr)), so that only per-sample
 * transcendental calls differ between host libm and device ocml.  Layout per unit type: seg.hip.
 * ---------------------------------------------------------------------------------------------- */
#define GDG_DS_LEN 32
#define GDG_IS_LEN 8
#define GDG_DP_LEN 32
#define GDG_JP_LEN 8

struct gdg_seg_unit {
    int type;
    int pad;
    int ip[8];                /* resolved parameters (numeric value / discrete index) */
    int jp[GDG_JP_LEN];       /* derived integers */
    double dp[GDG_DP_LEN];    /* derived doubles */
    double *ds;
    int *is;
    double *hist;
    const double *tab;        /* scan tables of the unit's constant-coefficient recurrences (powers of the 8-sample chunk map), built on the
                               * host at plan time -- they depend on the coefficients only -- and shared by all units with the same ones */
};

/* scan tables (seg.hip: lin_scan / lin2_scan); layouts shared with the host builder in api_plan.cpp.  A thread's chunk has GDG_CHK samples:
 * 8 in the general segment kernel (1024 threads per frame), 16 in the two-per-CU kernel for the batch block size (512 threads,
 * seg.hip compiled with -DSEG_FAST); the layouts below take the chunk size as a parameter because the host builds both. */
#ifndef GDG_CHK
#define GDG_CHK 8                 /* samples per thread at the batch block size (8192 / 1024) */
#endif
#define GDG_CHK_FAST 16           /* ... of the 512-thread kernel */
#define LT_W_(c) 0                /* [c]  dot weights */
#define LT_ST_(c) (c)             /* [10] A^(2^k), k = 0..9 */
#define LT_PA_(c) ((c) + 10)      /* [16] A^(q + 1), q = lane & 15 */
#define LT_PB_(c) ((c) + 26)      /* [32] A^(lane - 31), lane = 32..63, at index lane - 32 */
#define LT_PC_(c) ((c) + 58)      /* [64] A^lane */
#define LT_SIZE_(c) ((c) + 122)
#define L2_W_(c) 0                /* [c][2]  dot weights (gH_i, gL_i) */
#define L2_ST_(c) (2 * (c))       /* [10][3] P^(2^k) */
#define L2_PA_(c) (2 * (c) + 30)  /* [16][3] */
#define L2_PB_(c) (2 * (c) + 78)  /* [32][3] */
#define L2_PC_(c) (2 * (c) + 174) /* [64][3] */
#define L2_SIZE_(c) (2 * (c) + 366)
#define LT_W LT_W_(GDG_CHK)
#define LT_ST LT_ST_(GDG_CHK)
#define LT_PA LT_PA_(GDG_CHK)
#define LT_PB LT_PB_(GDG_CHK)
#define LT_PC LT_PC_(GDG_CHK)
#define LT_SIZE LT_SIZE_(GDG_CHK)
#define L2_W L2_W_(GDG_CHK)
#define L2_ST L2_ST_(GDG_CHK)
#define L2_PA L2_PA_(GDG_CHK)
#define L2_PB L2_PB_(GDG_CHK)
#define L2_PC L2_PC_(GDG_CHK)
#define L2_SIZE L2_SIZE_(GDG_CHK)

struct gdg_seg_chan {
    const double *src;
    double *dst;
    double *scratch;          /* one frame of per-channel global scratch */
    int unit_begin;
    int unit_count;
    int flags;                /* GDG_SRC_IS_INPUT / GDG_DST_IS_OUTPUT */
    int wave_mask;            /* WAVE: bit u (u < 15) = unit u of the segment carries state from frame to frame (it meets its predecessor frame; units
                               * from the 16th on always do); bit 16 + u = it reads that state through sc1 loads only (no acquire fence at its
                               * hand-off); bit 31 = some unit of the segment stores that state with plain stores: hand-offs write the XCD's L2 back */
    int *wave;                /* [8 x unit_count] frame counters of the units of this channel's segment (seg.hip, WAVE); zero between launches */
};

/* oversampling tables shared by all channels (device memory) */
struct gdg_os_tables {
    const double *taps2;      /* 77  */
    const double *taps4;      /* 155 */
    const double *lanczos2;   /* [1][6] weights of the half-sample phase */
    const double *lanczos4;   /* [3][6] weights of phases 1/4, 2/4, 3/4 */
    /* the decimator taps again, phase-major and zero padded for the register-blocked decimator of seg.hip:
     * tp[r][e] = taps[F (e - GDG_OS_PADLO(F)) - r] where that index exists, else 0 */
    const double *tapsP2;     /* [2][GDG_OS_NE(2)] */
    const double *tapsP4;     /* [4][GDG_OS_NE(4)] */
};
#define GDG_OS_TAPS(F) ((F) == 2 ? 77 : 155)
#define GDG_OS_BACK(F) ((GDG_OS_TAPS(F) - 1 + (F) - 1) / (F))      /* 38 / 39 */
#define GDG_OS_R(F) ((F) == 2 ? 4 : 2)                              /* consecutive outputs per thread */
#define GDG_OS_NC 48                                                /* slots per phase walked by a thread (>= BACK + R, multiple of 8) */
#define GDG_OS_PADLO(F) (GDG_OS_NC - 1 - GDG_OS_BACK(F))
#define GDG_OS_NE(F) (GDG_OS_NC + GDG_OS_R(F) - 1 + 1)              /* table entries per phase (+1: even) */

/* epoch: a number no other WAVE launch of the context carries (marks that must not be mistaken for an earlier launch's).
 * d_wave_ticket != NULL and n_frames > 1: a workgroup per FRAME and channel, the frames of a channel meeting unit by unit (seg.hip, WAVE) --
 * for windows of channel counts that leave most of the chip idle; the counter (zero before the first launch, zero after every launch)
 * belongs to this launch slot alone */
hipError_t gdg_launch_seg(const gdg_seg_chan *d_chans, int n_chans, const gdg_seg_unit *d_units, int frames, int n_frames, gdg_shift shift,
                          gdg_os_tables os, int *d_error, hipStream_t s, int *d_wave_ticket = nullptr, int epoch = 0, int ahead = 0,
                          const int *d_ahead_list = nullptr, int n_ahead = 0);
/* one frame per launch (n_frames == 1), general kernel: d_ahead_list names n_ahead reverbs (indices into d_units) of LATER segment steps of the
 * call whose wet path this launch makes with extra workgroups (seg.hip REVERB_AHEAD); ahead != 0: reverbs whose descriptor says so (ip[7])
 * only mix -- an earlier launch of the call made theirs */
/* the same for segments that only hold units the two-per-CU kernel runs (gdg_segf_supported) on frames of 8192 samples */
hipError_t gdg_launch_segf(const gdg_seg_chan *d_chans, int n_chans, const gdg_seg_unit *d_units, int frames, int n_frames, gdg_shift shift,
                           gdg_os_tables os, int *d_error, hipStream_t s, int *d_wave_ticket = nullptr, int epoch = 0, int ahead = 0,
                           const int *d_ahead_list = nullptr, int n_ahead = 0);
int gdg_segf_supported(int unit_type);
/* per-frame calls of few channels: a channel's frame on TWO workgroups (seg.hip compiled with -DSEG_TILE; same bits as gdg_launch_seg).  The
 * segments may hold the unit types gdg_segt_supported says, without oversampling, and at most 32 exchange ids in all (gdg_segt_exchanges per
 * unit); d_ticket: a counter that is zero between launches; d_xch: gdg_segt_xch_words() 8-byte words per descriptor, zero before first use;
 * epoch: a number no earlier launch used on these words; d_ahead_list / n_ahead as in gdg_launch_seg */
hipError_t gdg_launch_segt(const gdg_seg_chan *d_chans, int n_chans, const gdg_seg_unit *d_units, gdg_shift shift, gdg_os_tables os, int *d_error,
                           hipStream_t s, int *d_ticket, int epoch, unsigned long long *d_xch, const int *d_ahead_list, int n_ahead);
int gdg_segt_supported(int unit_type);
int gdg_segt_exchanges(int unit_type);
size_t gdg_segt_xch_words(void);
/* an oversampled shaper (overdrive / distortion / excess at 2 x or 4 x) as a launch of its own, one workgroup per (channel, frame, tile): the
 * descriptors are segment descriptors whose unit_begin names the shaper; d_flags: one int per channel, any value but `epoch` (seg.hip) */
hipError_t gdg_launch_os_tiles(int factor, const gdg_seg_chan *d_chans, int n_chans, const gdg_seg_unit *d_units, int frames, int n_frames,
                               gdg_shift shift, gdg_os_tables os, int *d_flags, int epoch, int *d_error, hipStream_t s,
                               const gdg_seg_chan *d_pre_chans = nullptr, int *d_arrive = nullptr);
/* d_pre_chans (n_frames == 1): descriptor i = the segment step in front of d_chans[i]'s shaper, a lone compressor -- the tiles' workgroups run it
 * themselves (that step is then not launched); d_arrive: one int per channel, zero between launches */
hipError_t gdg_launch_os_debug(int factor, const double *d_in, int n, double *d_hist, double *d_up, double *d_down, gdg_os_tables os, hipStream_t s);
/* 1 when seg.hip implements the unit type */
int gdg_seg_supported(int unit_type);

/* ------------------------------------------------------------------------------------------------
 * Spatializer (spat.hip): per-channel constants derived on the host (spatializer.go:170-240).
 * mode 0: no inter-aural delay, 1: left ear delayed (delayTime > 0), 2: right ear delayed.
 * ---------------------------------------------------------------------------------------------- */
struct gdg_spat_chan {
    double fac_left, fac_right, w_early, w_late;
    int mode, early, late, pad;
};
/* one launch: mix of `frames` samples (right = left + out_stride) reading the history d_hist_read, and the new history (last H inputs of
 * every channel) into d_hist_write -- two different buffers, swapped by the caller from block to block */
hipError_t gdg_launch_spatializer(const gdg_spat_chan *d_chans, int nch, const double *d_in, int in_stride, const double *d_hist_read,
                                  double *d_hist_write, int H, double *d_out_lr, int out_stride, int frames, hipStream_t s);

/* ------------------------------------------------------------------------------------------------
 * Tuner (tuner.hip): one 96000-sample ring per channel; analysis = 262144-point real FFT
 * autocorrelation as a four-step FFT over HBM (tuner/tuner.go:379-577).
 * ---------------------------------------------------------------------------------------------- */
#define GDG_TUNER_RING 96000          /* tuner/tuner.go:16 */
#define GDG_TUNER_FFT 262144          /* nextpow2(2 * 96000), tuner.go:388-390 */
/* seq: the analysis this record belongs to -- written LAST, at system scope, so that a host that finds the current number in a record of
 * mapped, coherent host memory may read the record without waiting for the stream (api_tuner_spat.cpp) */
struct gdg_tuner_out { double frequency; int note_index; int cents; unsigned seq; int pad; };
hipError_t gdg_launch_tuner_enqueue(double *d_rings, int nch, int wp, const double *d_samples, int stride, int frames, hipStream_t s);
hipError_t gdg_tuner_tables_create(double2 **d_tw_n, double2 **d_tw_m);
int gdg_tuner_short_ok(double sample_rate, double lowest_note_frequency);
/* parts > 1: a channel's blocks over `parts` workgroups, partial sums through d_partial ([nch][parts][4096] complex) */
int gdg_tuner_short_parts(int nch);
hipError_t gdg_launch_tuner_short(const double *d_rings, int nch, int wp, double sample_rate, const double2 *tw4096, const double2 *tw2_4096,
                                  const double *d_note_freqs, int n_notes, gdg_tuner_out *d_out, double2 *d_partial, int parts, hipStream_t s, unsigned seq = 0);
hipError_t gdg_launch_tuner_analyze(const double *d_rings, int nch, int wp, double sample_rate, double2 *d_work,
                                    const double2 *d_tw_n, const double2 *d_tw_m, const double2 *d_tw512, const double2 *d_tw256,
                                    const double *d_note_freqs, int n_notes, gdg_tuner_out *d_out, hipStream_t s, unsigned seq = 0);

/* ------------------------------------------------------------------------------------------------
 * io.hip: the data formats either side of the path: wave sample codecs, resample.Time,
 * level meters.  Planar float64 [channels][per] on the sample side, interleaved little-endian bytes on
 * the file side.
 * ---------------------------------------------------------------------------------------------- */
#define GDG_METER_SEG 8192
struct gdg_meter_rec { double current, peak; unsigned long long counter; int enabled, pad; };
hipError_t gdg_launch_wave_decode(int fmt, const void *d_bytes, size_t per, unsigned channels, double *d_out, hipStream_t s);
/* What an encode launch does beyond the plain encoder (io.hip, the encode launchers): `trim`, every sample times its port's gain -- one rounded
 * product (trim.h; include/gdg.h, gdg_batch_set_trim) -- and `dither`, TPDF dither of the LPCM formats, a sample's noise a function of
 * (seed, port, index) alone (dither.h; gdg_batch_set_dither).  The callers' rules set the two (a gain of 1.0 or no gains: no trim; mode 0
 * or an IEEE format: no dither); a launcher reads only what a switch that is on needs.  {} is the plain encoder. */
struct gdg_dither_rows { unsigned long long seed, first; unsigned port_base, n_chain; };
struct gdg_encode_mode {
    bool trim, dither;
    const double *d_gains;       /* trim, rows: row r has gain d_gains[r] (device memory) */
    double gain[2];              /* trim, the master: left and right; stand-alone: gain[0] */
    gdg_dither_rows dz;          /* dither, rows: row r is sample `first` .. of port gdg_dither_row_port(port_base, n_chain, r); the master: seed and
                                  * the piece's `first` (left is port 0xfffffffd, right 0xfffffffe); stand-alone: seed, first and port_base = the port */
};
/* stand-alone: planar [channels][per] -> interleaved bytes; trimmed or dithered: mono, d_in 8-byte aligned (unaligned buffers and n % 4 go one sample per thread) */
hipError_t gdg_launch_wave_encode(int fmt, const double *d_in, size_t per, unsigned channels, void *d_bytes, const gdg_encode_mode &m, hipStream_t s);
/* rows of one strided array -> compact encoded rows (row_len % 4 == 0); trimmed IEEE64 needs d_bytes 8-byte aligned */
hipError_t gdg_launch_wave_encode_rows(int fmt, const double *d_in, size_t row_stride, size_t row_len, unsigned n_rows, void *d_bytes,
                                       const gdg_encode_mode &m, hipStream_t s);
/* many mono pieces in one launch (the batch run's streamed upload): piece r = `count` samples of format `fmt` at `src` -> dst */
/* stride > 1: the piece holds interleaved frames of `stride` channels, of which channel `offset` is decoded (0 / 1: mono, as above) */
struct gdg_decode_row { const unsigned char *src; double *dst; unsigned count; int fmt; unsigned stride, offset; };
hipError_t gdg_launch_wave_decode_rows(const gdg_decode_row *d_rows, int n_rows, unsigned max_count, hipStream_t s);
/* resample.Time over spans of several files in one launch (the streamed batch run; io.hip resample_span_kernel) */
struct gdg_resample_span {
    const double *src;           /* source frames [src_first, src_first + src_count) of the file */
    double *dst;                 /* output samples [out_first, out_first + count) */
    double *carry;               /* receives the last `keep` (<= 256) frames of src */
    long long src_first, n, out_first;
    double dx;
    unsigned count, src_count, keep, pad;
};
hipError_t gdg_launch_resample_spans(const gdg_resample_span *d_spans, int n_spans, unsigned max_count, hipStream_t s);
/* The fan-out forms of the two launches above (a batch job with a source map, gdg_batch_set_sources): a root's piece is read and
 * converted -- a root's span resampled -- ONCE and stored to n_dst rows, d_table[dst_first .. dst_first + n_dst): the root's own row and
 * its readers'.  The table travels in the same upload as the descriptors.  vec: every row of the fan is 16-byte aligned (the word-wise
 * path of the decoder).  The single-destination kernels are untouched and serve every step without a reader. */
struct gdg_decode_fan { const unsigned char *src; unsigned count; int fmt; unsigned stride, offset; unsigned dst_first, n_dst; unsigned vec, pad; };
hipError_t gdg_launch_wave_decode_fans(const gdg_decode_fan *d_fans, double *const *d_table, int n_fans, unsigned max_count, hipStream_t s);
struct gdg_resample_fan {
    gdg_resample_span span;      /* span.dst is not used: the rows are the table's */
    unsigned dst_first, n_dst;
};
hipError_t gdg_launch_resample_fans(const gdg_resample_fan *d_fans, double *const *d_table, int n_fans, unsigned max_count, hipStream_t s);
hipError_t gdg_launch_resample_time(const double *d_in, int n, double dx, double *d_out, int n_out, hipStream_t s);
hipError_t gdg_launch_meter(const double *d_rows, size_t stride, int n_ports, int n, gdg_meter_rec *d_state,
                            double decay, unsigned long long hold, hipStream_t s);

/* dst_a[i] += src[i]; dst_b[i] += src[i]  (the aux input of the spatializer, spatializer.go:300-310) */
hipError_t gdg_launch_add_aux(double *d_a, double *d_b, const double *d_src, int n, hipStream_t s);
/* the master of one piece of a sharded job (gdg_batch_finish_master, gdg_batch_finish_master_slice): d_slab = [left_0 .. left_{G-1} | right_0 .. right_{G-1} | aux] rows of
 * `stride` samples; per side ((p_0 + p_1) + ... + p_{G-1}) + aux, encoded into n * width bytes at d_left_bytes / d_right_bytes; d_sums
 * non-null: the float64 sums as well, left at d_sums, right at d_sums + sums_stride (the meters read them), taken before trim and dither.  n a multiple of 4: a ragged piece comes with zeros up to the next one. */
hipError_t gdg_launch_finish_master(int fmt, const double *d_slab, size_t stride, int n_shards, int has_aux, size_t n, void *d_left_bytes,
                                    void *d_right_bytes, double *d_sums, size_t sums_stride, const gdg_encode_mode &m, hipStream_t s);
hipError_t gdg_launch_metronome(const double *d_tick, unsigned n_tick, const double *d_tock, unsigned n_tock, double *d_out, int n,
                                unsigned sc0, unsigned tc0, unsigned spb, unsigned beats, unsigned j0, hipStream_t s);
/* the render report (include/gdg.h): one gdg_block_stats per block of `block` samples (the last of a row may be short) of n_rows rows of
 * `samples` samples, row r at d_rows + r * row_stride (8-byte aligned, row_stride >= samples), into d_records[r][ceil(samples / block)] */
hipError_t gdg_launch_block_stats(const double *d_rows, size_t row_stride, unsigned n_rows, size_t samples, unsigned block, void *d_records, hipStream_t s);
/* the band spectrum (include/gdg.h; fir.hip, spectrum_kernels.h): per block of 8192 samples of every row (the last of a row may be short: zero-padded)
 * the powers of bands.n_bands bands into d_bands[r][ceil(samples / 8192)][n_bands].  d_win: the 8192 window weights; tw, tw2: the 4096-point tables */
hipError_t gdg_launch_block_spectrum(const double *d_rows, size_t row_stride, unsigned n_rows, size_t samples, const double *d_win, const double2 *tw4096,
                                     const double2 *tw2_4096, const gdg_spectrum_bands &bands, double *d_bands, hipStream_t s);
/* the alignment report (include/gdg.h; fir.hip, align_kernels.h): per block of 8192 samples (the last of a row may be short: zero-padded) and
 * per entry of `pairs` one gdg_block_align into d_records[port][ceil(samples / 8192)].  Ports below n_chain are the rows of their number, the
 * ports from n_chain on the rows from tail_row on (row r at d_rows + r * row_stride); tw8192: the 8192-point table */
hipError_t gdg_launch_block_align(const double *d_rows, size_t row_stride, unsigned n_chain, unsigned tail_row, unsigned n_ports, size_t samples,
                                  const gdg_align_pairs &pairs, const double2 *tw8192, void *d_records, hipStream_t s);
/* the true-peak record (include/gdg.h; io.hip, true_peak_kernels.h): per block of 8192 samples (the last of a row may be short: just shorter) of
 * n_rows rows one gdg_block_true_peak into d_records[r][ceil(samples / 8192)]; taps: the table of true_peak_taps.h, passed by value */
hipError_t gdg_launch_block_true_peak(const double *d_rows, size_t row_stride, unsigned n_rows, size_t samples, const gdg_true_peak_table &taps, void *d_records,
                                      hipStream_t s);
/* the blend outputs (include/gdg.h; io.hip, blend_kernels.h; the arithmetic, the table and its view: blend.h): row b of d_out (row b at d_out + b *
 * out_stride) is the sum of blend b's terms over `samples` samples of the rows of d_rows, in term order.  The view's table lies in device memory
 * and has been checked by the caller.  The kernel by what the view holds: taps = filtered terms, else delays = delayed terms, else plain ones.
 * d_history: null (+0.0 in front of sample 0) or, per row, the GDG_BLEND_MAX_DELAY samples in front of sample 0 at d_history + r * hist_stride
 * (hist_stride >= GDG_BLEND_MAX_DELAY); read, never written, and not looked at without delays.  Rows 8-byte aligned, strides >= samples;
 * d_out overlaps neither the rows nor the history. */
struct gdg_blend_view;
hipError_t gdg_launch_blend(const gdg_blend_view &view, const double *d_rows, size_t row_stride, size_t samples, const double *d_history, size_t hist_stride,
                            double *d_out, size_t out_stride, hipStream_t s);
/* the last GDG_BLEND_MAX_DELAY of `samples` samples (samples >= GDG_BLEND_MAX_DELAY) of rows 0 .. n_rows - 1 into d_history[n_rows][GDG_BLEND_MAX_DELAY] */
hipError_t gdg_launch_blend_history_save(const double *d_rows, size_t row_stride, size_t samples, unsigned n_rows, double *d_history, hipStream_t s);
/* the delivery (include/gdg.h, DELIVERY; io.hip, deliver_kernels.h; deliver.h): n_rows rows of `samples` session samples (a positive multiple of
 * `factor`, 2 or 4) -> rows of samples / factor samples at d_out + r * out_stride: the factor's anti-aliasing FIR (d_taps: its 77 or 155 expanded
 * taps in device memory), every factor-th sample, times ATTENUATION_HALF_DECIBEL.  d_history: null (+0.0 in front of sample 0) or [n_rows][154],
 * the session samples in front of the launch; read, never written.  Rows 8-byte aligned; d_out overlaps neither the rows nor the history. */
hipError_t gdg_launch_deliver_rows(int factor, const double *d_rows, size_t row_stride, size_t samples, unsigned n_rows, const double *d_taps, const double *d_history,
                                   double *d_out, size_t out_stride, hipStream_t s);
/* ... and behind it, before the rows are written again: the rows' last 154 samples into d_history[n_rows][154]; a launch of fewer moves the old ones up */
hipError_t gdg_launch_deliver_history_save(const double *d_rows, size_t row_stride, size_t samples, unsigned n_rows, double *d_history, hipStream_t s);
/* the ratio stage behind it (io.hip, deliver_ratio_kernels.h): n_rows rows of `samples` intermediate samples, the job's [first, first + samples), ->
 * the outputs ceil(first up / down) <= n < ceil((first + samples) up / down) at d_out + r * out_stride, then +0.0 up to pad_to samples (0: none).
 * d_tapsT: the ratio's table as [T][up] in device memory; d_history: null or [n_rows][127], read, never written. */
hipError_t gdg_launch_deliver_ratio(int up, int down, const double *d_rows, size_t row_stride, size_t samples, unsigned long long first, unsigned n_rows, const double *d_tapsT,
                                    const double *d_history, double *d_out, size_t out_stride, size_t pad_to, hipStream_t s);
/* ... and behind it: the rows' last 127 samples into d_history[n_rows][127]; a launch of fewer moves the old ones up */
hipError_t gdg_launch_deliver_ratio_history_save(const double *d_rows, size_t row_stride, size_t samples, unsigned n_rows, double *d_history, hipStream_t s);
/* the records of the delivered rows (io.hip, delivered_kernels.h; include/gdg.h, DELIVERED RECORDS): n_rows rows of `samples` float64 cut into
 * n_blocks blocks by d_span[0 .. n_blocks] (device memory; ascending from 0 to `samples`, lengths 1 to 16384: held by the caller against the
 * host's copy) -> d_records[n_rows][n_blocks] of 40 bytes.  d_history: null or [n_rows][23], read, never written. */
hipError_t gdg_launch_block_delivered(const double *d_rows, size_t row_stride, unsigned n_rows, size_t samples, const unsigned long long *d_span, unsigned n_blocks,
                                      const double *d_history, const gdg_true_peak_table &taps, void *d_records, hipStream_t s);
/* ... and behind it: the last 23 samples of (history ++ rows) into d_history[n_rows][23] */
hipError_t gdg_launch_delivered_history_save(const double *d_rows, size_t row_stride, size_t samples, unsigned n_rows, double *d_history, hipStream_t s);
/* the blend fit's records (include/gdg.h, FIT; io.hip, fit_kernels.h): per fit and block of `block` samples (the last of a row may be short)
 * one gdg_block_fit, d_records[n_fits][ceil(samples / block)].  A fit is target | terms | port[8] (blend.h, FitSet): h_table is the host's copy
 * of the device's d_table, held against n_rows before anything is launched. */
hipError_t gdg_launch_block_fit(const double *d_rows, size_t row_stride, unsigned n_rows, size_t samples, unsigned block, const int *h_table, const int *d_table,
                                unsigned n_fits, void *d_records, hipStream_t s);
/* the Gram records (include/gdg.h, GRAM; gram.hip, gram_kernels.h): per block of `block` samples (the last of a row may be short) the lower
 * triangle of the Gram matrix of the n_ports listed rows, d_records[ceil(samples / block)][n_ports (n_ports + 1) / 2].  h_ports is the host's
 * copy of the device's d_ports, held against n_rows before anything is launched. */
hipError_t gdg_launch_block_gram(const double *d_rows, size_t row_stride, unsigned n_rows, size_t samples, unsigned block, const int *h_ports, const int *d_ports,
                                 unsigned n_ports, void *d_records, hipStream_t s);
/* the tap-fit records (include/gdg.h, TAPFIT; gram.hip, tapfit_kernels.h): per block of `block` samples (the last of a row may be short) and
 * fit the lower triangle of the Gram matrix of its K T + 1 shifted rows, d_records[ceil(samples / block)][D].  h_table is the host's copy of
 * the device's d_table (blend.h, gdg_tapfit_table), held against the limits and n_rows before anything is launched. */
hipError_t gdg_launch_block_tapfit(const double *d_rows, size_t row_stride, unsigned n_rows, size_t samples, unsigned block, const int *h_table, const int *d_table,
                                   unsigned n_fits, void *d_records, hipStream_t s);
/* the transfer records (include/gdg.h, TRANSFER; fir.hip, transfer_kernels.h): per block of 8192 samples (the last of a row may be short:
 * zero-padded) and (port, target) pair the auto-spectra and the cross-spectrum in groups of D bins, d_records[ceil(samples / 8192)][n_pairs]
 * [4096 / D + 1][4].  h_table is the host's copy of the device's d_table (blend.h, gdg_transfer_table: port, target per pair, then D), held
 * against the limits (blend.h, GDG_TRANSFER_*) and n_rows before anything is launched; tw8192: the 8192-point table */
hipError_t gdg_launch_block_transfer(const double *d_rows, size_t row_stride, unsigned n_rows, size_t samples, const int *h_table, const int *d_table,
                                     unsigned n_pairs, const double2 *tw8192, void *d_records, hipStream_t s);

/* compile.hip: power-amp filter compilation */
hipError_t gdg_launch_filter_reduce(const double *d_taps, int n, unsigned order, double2 *work_a, double2 *work_b, double2 *work_pos, double *d_out,
                                    hipStream_t s);
void gdg_filter_reduce_sizes(int n, unsigned order, size_t *work_points, size_t *pos_points);
/* d_partial: 257 doubles of scratch */
hipError_t gdg_launch_normalize_scale_add(const double *d_src, int n, double compensation, double level, double *d_partial, double *d_composite,
                                          hipStream_t s);

/* state.hip: channel state saved / loaded (api_state.cpp) -- `bytes` from src to dst for every piece, zeros where src is null.  A piece
 * occupies ceil(bytes / GDG_STATE_CHUNK) chunks, the first of them d_first[i] (ascending); n_chunks in all, a workgroup each. */
#define GDG_STATE_CHUNK 16384
struct gdg_state_piece { const void *src; void *dst; unsigned long long bytes; };
hipError_t gdg_launch_state_copy(const gdg_state_piece *d_pieces, const unsigned *d_first, int n_pieces, unsigned n_chunks, hipStream_t s);

/* state.hip: the payload digest of a checkpoint container (include/gdg.h states the function; api_checkpoint.cpp finishes it).  Granule g
 * (16 bytes: the little-endian 64-bit words a, b) gives u = mix(a + (g + 1) K, M0, 32), v = mix(b ^ u, M1, 29) with mix(x, M, r) = (x M) ^
 * ((x M) >> r) mod 2^64; the launch leaves per workgroup {sum of u mod 2^64, XOR of v} in d_partials[2 * group ..].  Sum and XOR commute,
 * so the two totals do not depend on `groups` (1 .. GDG_DIGEST_GROUPS) or on which workgroup met which granule. */
#define GDG_DIGEST_K  0x9e3779b97f4a7c15ull
#define GDG_DIGEST_M0 0xff51afd7ed558ccdull
#define GDG_DIGEST_M1 0xc4ceb9fe1a85ec53ull
#define GDG_DIGEST_GROUPS 2048
hipError_t gdg_launch_state_digest(const void *d_payload, unsigned long long granules, unsigned long long *d_partials, int groups, hipStream_t s);

#endif
