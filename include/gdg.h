/*
 * gdg.h -- C-ABI of libgdg.so: the MI355X-native (HIP, gfx950) batch implementation of
 * go-dsp-guitar's per-channel effects pipeline.
 *
 * This is the drop-in boundary.  A cgo shim (go-dsp-guitar_amd/go/, shown in INTEGRATION.md)
 * keeps the reference's Go interfaces effects.Unit (effects/effects.go:83-91) and
 * signal.Chain (signal/signal.go:21-36) and forwards to the entry points below; name lookup,
 * range checks and error strings stay on the host side, only resolved integers, taps and
 * sample buffers cross the ABI.  Plain pointers and sizes only; no C++ or torch types.
 *
 * One context = one GPU = one shard of channels.  Channels are independent, so an N-GPU
 * host creates N contexts and never needs a collective.
 *
 * Conventions
 *   - every function returns GDG_OK (0) or a negative GDG_ERR_* code; gdg_last_error() gives
 *     a message for the last failure on that context;
 *   - a context is NOT internally synchronised: one call at a time per context (the reference's N worker goroutines meet in a
 *     rendezvous above the ABI -- go-dsp-guitar_amd/go/signal, host/gdg_host.cpp -- and the last arrival makes the one call;
 *     control-plane setters take the same lock).  Different contexts (different GPUs) are independent;
 *   - there is NO CPU fallback: without a usable HIP device gdg_ctx_create fails with
 *     GDG_ERR_NO_DEVICE, and a chain that contains something the HIP path cannot run fails
 *     with GDG_ERR_UNSUPPORTED instead of silently computing elsewhere;
 *   - unit_type values are the reference's UNIT_* iota (effects/effects.go:21-43);
 *   - parameter indices follow the declaration order of each unit's create*() table in
 *     effects/<unit>.go; numeric parameters carry their int32 value, discrete parameters the
 *     index into the reference's DiscreteValues list (e.g. oversampling: 0 "- NONE -", 1 "2", 2 "4").
 */
#ifndef GDG_H
#define GDG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GDG_OK                0
#define GDG_ERR_INVALID      -1   /* bad handle, index or argument */
#define GDG_ERR_UNSUPPORTED  -2   /* valid in the reference, not runnable on the HIP path (yet) */
#define GDG_ERR_HIP          -3   /* a HIP runtime call failed */
#define GDG_ERR_NO_DEVICE    -4   /* no usable gfx950 device */
#define GDG_ERR_NOMEM        -5

enum gdg_unit_type {              /* effects/effects.go:21-43 */
    GDG_UNIT_SIGNALGENERATOR = 0, GDG_UNIT_NOISEGATE, GDG_UNIT_BANDPASS, GDG_UNIT_AUTOWAH,
    GDG_UNIT_AUTOYOY, GDG_UNIT_COMPRESSOR, GDG_UNIT_OCTAVER, GDG_UNIT_EXCESS, GDG_UNIT_FUZZ,
    GDG_UNIT_OVERDRIVE, GDG_UNIT_DISTORTION, GDG_UNIT_TONESTACK, GDG_UNIT_CHORUS,
    GDG_UNIT_FLANGER, GDG_UNIT_PHASER, GDG_UNIT_TREMOLO, GDG_UNIT_RINGMODULATOR,
    GDG_UNIT_DELAY, GDG_UNIT_REVERB, GDG_UNIT_POWERAMP, GDG_UNIT_CABINET, GDG_UNIT_COUNT
};

#define GDG_MAX_PARAMS 8

typedef struct gdg_ctx gdg_ctx;

/* ---- library / context ----------------------------------------------------------------------- */

/* "gdg <version> gfx950 hip" */
const char *gdg_version(void);

/* Number of HIP devices visible to the process (0 when there is none / no driver). */
int gdg_device_count(void);

/*
 * Create the shard of n_channels channels on HIP device `device`.  max_frames bounds the
 * frames argument of gdg_process* (the reference's batch loop uses BLOCK_SIZE = 8192,
 * controller/controller.go:36).  Replaces: N x signal.CreateChain (controller.go:3267-3269),
 * spatializer.Create (:3273) and tuner.Create (:3279) for this shard.
 */
int gdg_ctx_create(int n_channels, int max_frames, int device, gdg_ctx **out);
int gdg_ctx_destroy(gdg_ctx *ctx);
const char *gdg_last_error(const gdg_ctx *ctx);
int gdg_ctx_channels(const gdg_ctx *ctx);
/*
 * Power amps whose composite filters are identical (same taps, same partition size) share ONE copy of the IR spectra in
 * HBM; the spectrum multiply-accumulate then streams it from L2 / MALL for all but the first channel (d < 1).
 * On by default (env GDG_SHARE_IR_SPECTRA=0 or enable = 0 turns it off for power amps prepared afterwards).  Results are
 * bit-identical either way.
 */
int gdg_ctx_share_ir_spectra(gdg_ctx *ctx, int enable);
/*
 * Launch-shape options of a context -- everything that used to be an environment variable of the process that loads the library.  The
 * variables still exist as DEBUG overrides of the defaults, read once when the context is made; a value set here wins.  Results never depend
 * on an option beyond the last bits (which association a sum takes); unknown keys and values out of range are GDG_ERR_INVALID.
 *   key                          values      meaning (default)
 *   fir_fused                    -1, 0, 1    spectrum multiply-accumulate inside the inverse transform's kernel: by channel count / never / always (-1)
 *   fir_split_max_channels       >= 0        with fir_fused = -1: launches of up to this many channels take the bin-tiled multiply-accumulate (192: with the
 *                                            sums made ahead, fir_premac, it is the faster shape up to there when a channel has two power amps)
 *   fir_split_max_channels_one_amp >= 0      ... and when the call has ONE power amp per channel the smaller of the two applies (112: with one amp the
 *                                            fused kernel wins at 128 channels, profiles/shape_sweep_r06.txt)
 *   fir_chain_adjacent_amps      0, 1        a power amp's inverse transform also makes the forward transform of the amp behind it (1)
 *   fir_premac                   0, 1        per-frame calls of few channels (the split launch shape): when a call ends, the sums of the NEXT frame's
 *                                            convolution over the partitions that are already in the delay line (7 of 8 at 65536 taps) are launched on a
 *                                            stream of their own and run beside the segments; the next call adds the newest term.  Speculative: any library
 *                                            call but a process call, gdg_ctx_synchronize and gdg_ctx_stream drops them.  Same bits either way (1)
 *   fir_premac_min_partitions    >= 1        ... for launches of at least this many partitions (channels x ceil(taps / 8192)) (384 = 48 channels x 65536
 *                                            taps: below, the two cross-stream hops cost more than they hide)
 *   fir_premac_min_partitions_two_amps >= 1  ... and when a channel has two or more power amps, the smaller of the two (320 = 40 channels x 65536 taps)
 *   stat_premac_launches_used    >= 0        a counter, not a setting: inverse-transform launches so far that continued sums made ahead (tests read it to
 *                                            see that the path under test is the one that ran; saturates; setting it sets the count) (0)
 *   stat_batch_device_kib        >= 0        a figure, not a setting: the capacity of the batch runs' device buffers in KiB, rounded up (what gdg_batch_release
 *                                            frees; saturates; a value set is replaced by the figure at the next read) (0)
 *   stat_batch_upload_bytes      >= 0        a counter, not a setting: bytes of input file data the last batch run call (or slice) moved to the device --
 *                                            with a source map (gdg_batch_set_sources) the roots' alone; reset when such a call begins (saturates; a
 *                                            value set is replaced by the figure at the next read) (0)
 *   stat_batch_resampled_samples >= 0        ... and the output samples for which that call evaluated resample.Time's Lanczos sum: once per sample
 *                                            of a root, however many channels read it (0)
 *   fir_premac_lds_bytes         -1 .. 65536 ... whose workgroups ask for this much LDS they never touch, so that they land on the CUs the segments leave
 *                                            idle instead of among the segments' waves; -1: 16384 below 120 channels, 49152 from there, 0 when a channel
 *                                            has fewer than 5 or more than 32 partitions (-1)
 *   fir_ahead_frames             0, 2 .. 4   per-frame calls of the fused launch shape (many channels, 8192-sample frames, every filter longer than one
 *                                            frame): a pass at the call's start sums, for a 1/T share of the channels, the terms of the next T frames that
 *                                            only need frames already in the delay line; the inverse kernels of those frames add the rest.  Every filter
 *                                            spectrum and delay-line slot is then read once per T frames instead of once per frame.  The sums belong to
 *                                            per-frame calls of one plan: a window call, a plan change (new filters, chains, options, frame size or
 *                                            channels) or a call that touches units, filters or the context's shape makes the next calls sum everything
 *                                            again; calls on caller data, codecs, tuner, spatializer and meters keep them.  Same bits either way
 *                                            (4; 0 or 1: never)
 *   fir_ahead_min_channels       >= 1        ... in launches (a channel group's power amp) of at least this many channels, when every channel's filter
 *                                            has enough partitions for the pass to move fewer bytes (K >= 5 at T = 4) (128)
 *   stat_fir_ahead_sums_used     >= 0        a counter, not a setting: channel frames so far whose inverse kernel continued sums made ahead, counted
 *                                            by the kernels on the device (reading it waits for the context's work; saturates; setting it sets
 *                                            the count) (0)
 *   share_ir_spectra             0, 1        = gdg_ctx_share_ir_spectra (1)
 *   seg_two_per_cu               0, 1        segments of in-place units on 8192-sample frames take the 512-thread kernel, two workgroups per CU (1)
 *   seg_two_per_cu_min_channels  >= 0        ... from this many channels per call on (128)
 *   seg_wave_max_channels        >= 0        windows (gdg_ctx_set_window) of up to this many channels per call: one workgroup per FRAME and channel, the
 *                                            frames of a channel meeting unit by unit -- fills the chip when the channels alone do not (448; 0: never)
 *   seg_wave_release_max_channels >= 0       ... but segments holding a unit whose state leaves the CU through plain stores (flanger, phaser, delay,
 *                                            fuzz, auto-yoy, auto-wah, band pass, octaver, noise gate: every hand-off writes the XCD's L2 back) only up
 *                                            to this many channels (112)
 *   seg_tile_max_channels        >= 0        per-frame calls of up to this many channels: a segment made of compressor, shapers without oversampling, tone
 *                                            stack, cabinet and chorus runs with a channel's 8192-sample frame on TWO workgroups -- the units of such a
 *                                            call are compute bound on one CU while most of the chip idles.  The scans keep the general kernel's
 *                                            association (a scan's sixteen wave totals meet in one place, eight of them through HBM): same bits.  Applies while the launch's
 *                                            workgroups -- 2 x channels + one per reverb whose wet path it carries -- stay within 224 of the 256 CUs (112; 0: never)
 *   seg_os_tiles_max_channels    >= 0        calls of up to this many channels run every 2 x / 4 x oversampled shaper as a launch of its own, one workgroup
 *                                            per (channel, frame, tile of 4096 / 2048 samples) instead of one per channel (192; 0: never)
 *   seg_os_tiles_prefix          0, 1        ... and when the step in front of such a launch is a lone compressor in every channel (compressor > 4 x overdrive:
 *                                            BASELINE config 3), a per-frame call runs that compressor inside the tiles' workgroups instead of launching it (1)
 *   seg_reverb_ahead_max_channels >= 0       per-frame calls of up to this many channels: the call's first segment launch also makes, with extra
 *                                            workgroups beside the channels' own, the wet path of every reverb of its LATER segment steps -- tapped
 *                                            sums and all-passes need nothing of the frame itself when every tap lies at least a frame back
 *                                            (8192-sample frames, rates from 42.7 kHz) -- and the reverb behind the power amps only mixes.  The limit
 *                                            applies to calls that also sum convolution terms ahead (fir_premac: its launches want the same idle CUs);
 *                                            without them up to 127 channels.  Same bits either way (72; 0: never)
 *   wave_spin_limit_ms           1 .. 600000 how long a workgroup of an in-launch hand-off (windows of few channels, tiles of an oversampled shaper) waits
 *                                            for its predecessor before the launch gives up: the wait ends, the context's error word is set and the next
 *                                            gdg_ctx_synchronize (or batch run) returns GDG_ERR_HIP -- the device never hangs.  RESULTS OF WINDOW CALLS ARE
 *                                            VALID ONLY AFTER A gdg_ctx_synchronize THAT RETURNED GDG_OK; after such an error the units' state is undefined
 *                                            (gdg_unit_reset them, or gdg_state_load a state saved before the failed call), the context itself
 *                                            stays usable (1000)
 *   debug_stall_unit             -1, handle  test hook: in the next windows' first frame this unit withholds its hand-off, so that the bounded wait can
 *                                            be seen to expire (-1)
 *   plan_patch                   0, 1        parameter changes patch the device descriptors in place instead of rebuilding the plan (1)
 *   scan_tables_max              >= 1        scan tables (one per distinct coefficient set) kept before a plan rebuild drops them all (1024)
 *   pcie_groups                  0 .. 16     channel groups of the host-buffer calls, 0 = by channel count (0)
 *   device_groups_default        0 .. 16     what gdg_ctx_set_overlap(ctx, 0) means, 0 = one group (0)
 *   copy_threads                 1 .. 256    host copy workers of the host-buffer paths and the batch run (8)
 *   numa                         0, 1, 2     copy workers on the CPUs, pinned slabs from the memory, of a NUMA node: 2 the node the caller runs on when
 *                                            they are made, 1 the device's node, 0 wherever the scheduler and hipHostMalloc put them (2; set it before
 *                                            the first host-buffer call -- slabs that exist stay where they are)
 *   tuner_poll_results           0, 1        gdg_tuner_analyze reads the result records (mapped host memory, each ending with its analysis number) as soon
 *                                            as they carry this call's number instead of waiting for the stream to drain (1)
 *   tuner_long_transform         0, 1        every tuner analysis through the reference's 262144-point transform pair (0)
 *   profile_attach               0, 1        the fused convolution launch records its own begin / end events (1)
 * Process-wide (the transforms' and the tuner's launchers have no context; set them before the first call that uses them):
 *   fft_half_lds_mask            0 .. 63     which 8192-point transforms run through ONE LDS buffer, two workgroups per CU (14)
 *   fir_forward_per_channel      0, 1        a window's forward transforms as one workgroup per channel from a chip's worth of channels on (1)
 *   fir_forward_wave_local       0 .. 3      8 x 1024 forward transform with wave-local sub-transforms (1)
 *   fir_mac_variant              0 .. 15     tile shape of the stand-alone multiply-accumulate (0)
 *   tuner_parts                  0 .. 24     workgroups per channel of the short-lag analysis, 0 = by channel count (0)
 * gdg_option_count / gdg_option_name enumerate the keys.
 */
int gdg_ctx_set_option(gdg_ctx *ctx, const char *key, long long value);
int gdg_ctx_get_option(gdg_ctx *ctx, const char *key, long long *value);
int gdg_option_count(void);
const char *gdg_option_name(int index);
/*
 * Where a PCI device hangs, from sysfs (what option "numa" uses): *node = <sysfs_root>/bus/pci/devices/<pci_bus_id>/numa_node (-1 when the
 * platform does not say), cpus[0 .. min(capacity, *n_cpus)) = the CPUs of <sysfs_root>/devices/system/node/node<N>/cpulist.  sysfs_root is
 * "/sys" outside tests.  No device needed.
 */
int gdg_numa_probe(const char *sysfs_root, const char *pci_bus_id, int *node, int *cpus, int capacity, int *n_cpus);
/* The hipStream_t all of this context's work is enqueued on (as void*), for event timing. */
void *gdg_ctx_stream(const gdg_ctx *ctx);
/* Block until everything enqueued so far has finished. */
int gdg_ctx_synchronize(gdg_ctx *ctx);
/* Give device memory the context no longer uses back to the device (entirely free chunks of the per-unit state arena, all but one spare).
 * Freeing device memory waits for the whole device, so the library never does it inside a process call; it happens here and whenever a plan
 * is rebuilt.  Blocks. */
int gdg_ctx_trim(gdg_ctx *ctx);

/* ---- effects units: effects.CreateUnit / Set*Value / state ----------------------------------- */

/* effects.CreateUnit(unitType) (effects/effects.go:443-516); parameters start at the reference's defaults. */
int gdg_unit_create(gdg_ctx *ctx, int channel, int unit_type, int *handle);
int gdg_unit_destroy(gdg_ctx *ctx, int handle);
/* Resolved value of one parameter (the host side has already done effects.go:144-384's checks).  Effective from the next process call, like the
 * reference's setter (effects/effects.go:283-345: a store under a mutex).  Cheap on a live context: the call itself stores the value; the next
 * process call re-derives that unit's constants and patches its descriptor on the device in place -- the launch plan is only rebuilt by changes of
 * a chain's layout (gdg_chain_set), of the frame size or rate, or by new filter taps.
 * "Cheap" has exceptions, all at the NEXT process call: (1) a value that moves the unit to another kernel -- any change of an oversampling
 * factor, a reverb leaving the in-place shape -- rebuilds the plan (~0.5 ms for 512 channels); (2) more than `scan_tables_max` distinct coefficient
 * sets since the last plan (a caller sweeping a tone stack through a thousand settings) rebuilds it once to drop the table cache; (3) a unit
 * whose constants cannot be derived (prepare fails) rebuilds it to report the error; (4) a value that re-makes a history the way the reference
 * does (a longer delay, a new band-pass order) waits for the stream and may take a new arena chunk: one device malloc and one fill of up to
 * 1 GiB, waited for.  Device memory is never FREED on this path (gdg_ctx_trim). */
int gdg_unit_set_param(gdg_ctx *ctx, int handle, int param_index, int32_t value);
int gdg_unit_get_param(gdg_ctx *ctx, int handle, int param_index, int32_t *value);
/*
 * Power amp only: the compiled composite FIR (what effects/poweramp.go:25-127 compile()
 * returns; Normalize/Reduce/Add stay on the host).  n_taps == 0 is filter.Empty (zeros out,
 * filter/filter.go:366-367).  Like the reference's recompile (poweramp.go:132-181) this
 * replaces the filter and therefore resets the convolution state.
 */
int gdg_unit_set_fir(gdg_ctx *ctx, int handle, const double *taps, int n_taps);
/* Zero all DSP state of a unit (what re-creating the unit does in the reference). */
int gdg_unit_reset(gdg_ctx *ctx, int handle);

/*
 * poweramp.compile on the device (effects/poweramp.go:25-127).  Slot i of the power amp holds the taps of
 * impulse response i at the current sample rate (filter.ImpulseResponses.CreateFilter(...).Coefficients(); NULL or length 0 =
 * "- NONE -"), its gain compensation FACTOR (filter/filter.go:127-138) and its `level_i` parameter in dB.  Per slot:
 * Reduce(target_order) when target_order > 0 and the slot is longer (filter.go:520-604), Normalize, Multiply(level); the
 * slots are then added in order (filter.go:167-236) and the composite becomes the unit's FIR exactly as gdg_unit_set_fir
 * would set it (including the state reset).  gdg_unit_get_fir reads the composite back (taps may be NULL to query n_taps).
 */
int gdg_unit_compile_fir(gdg_ctx *ctx, int handle, int n_filters, const double *const *taps, const int *lengths,
                         const double *gain_compensation, const int32_t *levels_db, uint32_t target_order);
int gdg_unit_get_fir(gdg_ctx *ctx, int handle, double *taps, int capacity, int *n_taps);

/*
 * signal.Chain slot list of one channel (signal/signal.go:52-157): handles in processing
 * order with their bypass flags.  Bypassed slots are skipped and do not advance their state
 * (signal.go:390-401).  State stays with the unit handle, not with the slot index.
 */
int gdg_chain_set(gdg_ctx *ctx, int channel, const int *handles, const uint8_t *bypass, int n);

/* ---- channel state: what a channel carries from one call to the next -------------------------------- */

/*
 * No reference counterpart.  Save the state of some channels into a blob and load it back into the same context (rollback after a failed
 * call, A/B rendering from one point) or into another one (another channel, another context or device, another channel count, window
 * or channel-group setting).  `channels` NULL: every channel of the context in order, `n` ignored.  A save writes one record per listed
 * channel in list order; a load applies record i to channels[i] and `n` must equal the blob's record count.  The _device variants take
 * a 16-byte-aligned buffer on the context's device (gdg_device_alloc).  Every call returns when the blob is complete or applied.
 *
 * State is what a call reads and an earlier call wrote: per unit its small state, FSM words and history ring (delay, chorus, flanger,
 * phaser, auto-yoy, reverb rings, oversampler histories) with the host's record of their layout; per power amp the overlap-save history,
 * the newest K delay-line slots in age order and the frame counter; per channel the spatializer's history row.  NOT state, not saved:
 * parameters and filter taps (they stay with the target's units: a parameter that changes no layout may differ), sums made ahead of the
 * frame, scan tables, spectra.  Out of scope of THIS blob: the tuner rings, meters, the metronome's counters and a streamed job's position
 * and resampler frames -- the checkpoint container (gdg_batch_stream_checkpoint, below) carries them beside this blob; a batch run's
 * other buffers hold nothing between two calls.
 *
 * A save has no side effects: it is ordered after everything queued on the context and keeps the sums made ahead, so a stream with
 * saves between its calls gives the same bits as one without.  A load is all or nothing: it lays the target's units out at the blob's
 * frame size and rate as a process call would, checks every record -- slot count, unit type per slot, ring layout (hist_key / hist_len),
 * oversampler frame size, band-pass order, the power amp's P / K / frame size / rate -- and only then writes.  A mismatch returns
 * GDG_ERR_INVALID naming channel, slot, unit type and key in gdg_last_error, and writes nothing.  A loaded delay line is rotated into
 * the target's ring, so a state saved per frame loads into a context with a window (gdg_ctx_set_window) and the other way round; a later
 * call at another frame size re-partitions it as usual.  A slot whose unit never ran is recorded as fresh and loads as a reset;
 * gdg_unit_set_fir after a load still resets.  Bypassed slots carry their state too.  A load drops whatever was summed ahead.
 *
 * Format (opaque; stable only within one format version, a blob of another version is rejected): little-endian; a 64-byte header
 * ("GDGSTATE", version 1, record count, frame size, rate, max_frames, metadata size, total size), per channel a record (slot count,
 * spatializer row) and its slot table (type, flags, layout keys, frame counter, payload offsets), then the payload at 16-byte alignment.
 * gdg_state_size gives the bytes a save of the same channels writes; a save into less capacity fails (*written = the size needed).
 */
int gdg_state_size(gdg_ctx *ctx, const int *channels, int n, size_t *bytes);
int gdg_state_save(gdg_ctx *ctx, const int *channels, int n, void *blob, size_t capacity, size_t *written);
int gdg_state_save_device(gdg_ctx *ctx, const int *channels, int n, void *d_blob, size_t capacity, size_t *written);
int gdg_state_load(gdg_ctx *ctx, const int *channels, int n, const void *blob, size_t bytes);
int gdg_state_load_device(gdg_ctx *ctx, const int *channels, int n, const void *d_blob, size_t bytes);

/* ---- processing: signal.Chain.Process for all channels of the shard at once ------------------- */

/*
 * One block of `frames` samples for every channel (what controller.process() fans out to its
 * N workers, controller/controller.go:2682-2705).  in[c] / out[c] are host buffers of `frames`
 * float64 each; the call stages them through pinned memory, runs the batch and blocks until
 * out is written.  in[c] is not modified.
 * `frames` may change from call to call (1 .. max_frames): like filter.Process (filter/filter.go:370-428, tail and transform
 * sizes depend on the filter length only) a power amp carries its convolution state across the change -- its delay line is
 * re-partitioned once per change.  A (frames, filter length) pair on which the reference itself panics (frames not a power
 * of two and a nextpow2(L)-sized block starting beyond the frame, filter.go:443-453) is rejected with GDG_ERR_UNSUPPORTED.
 */
int gdg_process(gdg_ctx *ctx, const double *const *in, double *const *out, int frames, uint32_t sample_rate);

/*
 * Same for a subset of the shard's channels: in[i] / out[i] belong to channel channels[i]; the
 * chains of all other channels are left untouched (their state does not advance).  This is what
 * the host shim's rendezvous falls back to when fewer than N Chain.Process calls are in flight.
 */
int gdg_process_subset(gdg_ctx *ctx, const int *channels, int n, const double *const *in, double *const *out,
                       int frames, uint32_t sample_rate);

/*
 * Staged variant for hosts that may not hand their own pointers to C (cgo's pointer rules):
 * gdg_staging_buffers returns two pinned host slabs (hipHostMalloc) whose row c (row_stride
 * float64 apart) belongs to channel c; every worker copies its frame into its input row,
 * gdg_process_staged runs the listed channels and fills their output rows.
 */
int gdg_staging_buffers(gdg_ctx *ctx, double **in, double **out, int *row_stride);
int gdg_process_staged(gdg_ctx *ctx, const int *channels, int n, int frames, uint32_t sample_rate);

/*
 * Same, device-resident: d_in / d_out are device pointers to [n_channels][frames] float64
 * (row-major, row stride = frames).  Enqueued on gdg_ctx_stream() and NOT synchronised;
 * d_in == d_out is not allowed.
 * Alignment: d_in and d_out must be 16-byte aligned (the kernels read and write the frames as sample pairs); any frame
 * length goes, odd ones included.  A pointer that is only 8-byte aligned -- a slice x[:, 1:] of an aligned tensor -- is
 * refused with GDG_ERR_INVALID and a message naming the pointer; nothing is launched and no state changes.
 */
int gdg_process_device(gdg_ctx *ctx, const double *d_in, double *d_out, int frames, uint32_t sample_rate);

/*
 * Time blocking for callers that hold several consecutive frames of every channel -- the batch run, whose files live in HBM
 * (controller.go:3076-3107 walks them 8192 samples at a time only because its buffers are that long).  A window of W frames per
 * channel and call: the units' state runs through the W frames in order, and every power amp reads its IR spectra and delay line
 * ONCE for all W frames (2 K + W - 1 spectrum reads instead of 2 K W; the sums keep their order and their arithmetic: the output is
 * bit-identical to W calls of gdg_process_device).
 * gdg_ctx_set_window: W in {1, 2, 4, 8, 16}; needs max_frames == 8192; may be called at any time, live convolution state moves into
 * the larger delay-line ring (K + W - 1 slots) like on a frame-size change.
 * gdg_process_window_device: d_in / d_out = [n_channels][row_stride] float64, frame j of channel c at c * row_stride + j * 8192;
 * frames_in_window in {1, 2, 4, 8, 16}, <= W (the tail of a file).  Enqueued on gdg_ctx_stream(), not synchronised.
 * Alignment: d_in and d_out must be 16-byte aligned and row_stride even, so that every row is; anything else is refused with
 * GDG_ERR_INVALID and a message naming the pointer or the stride, as in gdg_process_device.
 */
int gdg_ctx_set_window(gdg_ctx *ctx, int frames_per_call);
/*
 * Channel groups of the device-resident calls (gdg_process_device, gdg_process_window_device) -- OPT-IN.  By default every call's
 * kernels run on gdg_ctx_stream(): work a caller enqueues on that stream after the call is ordered after them.  With groups > 1 the
 * channels are cut into `groups` contiguous groups whose kernels run on streams of their own and are NOT joined at the end of the
 * call, so one group's latency-bound segment kernel overlaps another group's HBM-bound convolution, also across calls (+7-10 % at 512
 * channels with two groups).  The price is the ordering contract: the context's stream is ordered after the groups only by the next
 * library call of any other kind (including gdg_ctx_stream() and gdg_ctx_synchronize()) -- fetch the stream AFTER the process call if
 * you enqueue your own work behind it.  groups: 1 ... 16; 0 = back to the default (one group, unless env GDG_DEVICE_GROUPS names a
 * count).
 */
int gdg_ctx_set_overlap(gdg_ctx *ctx, int groups);
int gdg_process_window_device(gdg_ctx *ctx, const double *d_in, double *d_out, size_t row_stride, int frames_in_window, uint32_t sample_rate);

/* Device memory helpers for callers that have no HIP runtime of their own (e.g. the Go shim). */
int gdg_device_alloc(gdg_ctx *ctx, size_t bytes, void **d_ptr);
int gdg_device_free(gdg_ctx *ctx, void *d_ptr);
int gdg_copy_to_device(gdg_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int gdg_copy_to_host(gdg_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
/* n_rows rows of row_len float64 from one strided device array to another (strides in float64), enqueued on the context's stream,
 * not synchronised: cuts an 8192-frame block out of whole files resident in HBM and puts a processed block back
 * (controller/controller.go:3088-3099) */
int gdg_copy_rows_device(gdg_ctx *ctx, double *d_dst, size_t dst_stride, const double *d_src, size_t src_stride, size_t row_len, size_t n_rows);

/* ---- the transforms underneath the power amp, stand-alone ------------------------------------ */

/*
 * fft.RealFourier / fft.RealInverseFourier (fft/fft.go:744-856, :863-990) as fir.hip computes them (packed-real Stockham
 * transforms in registers + LDS): n real samples <-> n / 2 + 1 complex bins (re, im interleaved; the other half is the
 * conjugate mirror the reference also stores).  n = 1 (the identity, fft/fft.go:765-768) or a power of two from 2 to 16384 (n <= 64: a small radix-2 kernel of
 * the same packed-real scheme, which is what lets the reference's own eight-point known answers, fft/fft_test.go:237-271, run on the
 * HIP transforms).  Forward unscaled, inverse scaled by 1 / n
 * (SCALING_DEFAULT); like the reference the inverse reads only the real parts of bins 0 and n / 2.  Host buffers, blocking.
 */
int gdg_fft_real(gdg_ctx *ctx, const double *samples, int n, double *spectrum);
int gdg_fft_real_inverse(gdg_ctx *ctx, const double *spectrum, int n, double *samples);

/*
 * Debug entry: oversampling.OversamplerDecimator (oversampling/oversampling.go:27-30) as the 2x / 4x units' LDS tiles compute it --
 * Oversample (:54-115: Lanczos-3 polyphase, 8 inputs of history) followed by Decimate of ITS output (:126-184: 77 / 155-tap
 * anti-aliasing filter, clip, stride-f pick, x 0.944...), with no waveshaper in between: exactly the sequence
 * oversampling/oversampling_test.go:84-128 checks, so the reference's own vectors run on the HIP tiles.
 * factor 2 or 4; n <= 8192 samples in; `state` = the object's state across calls, 8 + (77 or 155) - 1 doubles, zeros = a fresh
 * object (in / out); oversampled: factor * n samples out (may be NULL); decimated: n samples out.  Host buffers, blocking.
 */
int gdg_debug_oversample_decimate(gdg_ctx *ctx, int factor, const double *in, int n, double *state, double *oversampled, double *decimated);

/* ---- per-kernel timing on the context's stream (HIP events), for bench.py's roofline ---------- */

enum gdg_kernel_kind {
    GDG_K_FIR_FWD = 0,   /* forward real FFT of the input partition -> frequency-domain delay line */
    GDG_K_FIR_MAC,       /* sum over partitions of FDL x IR spectra (the HBM-bound kernel) */
    GDG_K_FIR_INV,       /* inverse real FFT, clip, write */
    GDG_K_SEGMENT,       /* fused per-sample units between FIR units */
    GDG_K_TUNER,
    GDG_K_SPATIALIZER,
    GDG_K_WAVE,          /* wave sample codecs */
    GDG_K_RESAMPLE,      /* resample.Time */
    GDG_K_METER,         /* level meters */
    GDG_K_FIR_MAC_CHAIN, /* GDG_K_FIR_MAC of a power amp that is followed by another one: the same kernel also makes the next amp's forward
                          * transform (fir_inv_kernel CHAIN); kept apart so that GDG_K_FIR_MAC times the plain kernel only */
    GDG_K_FIR_AHEAD,     /* per-frame calls of many channels: the pass that sums the older partitions' terms of the next frames ahead
                          * (option fir_ahead_frames) */
    GDG_K_COUNT
};
/* enable == 1: bracket every kernel launch with a HIP event pair from now on (costs a few microseconds per launch);
 * enable == 1 << (kind + 1) (or-able): only the launches of those kernel kinds; 0: off.
 * The fused convolution launch (GDG_K_FIR_MAC / GDG_K_FIR_MAC_CHAIN) carries its two events itself: they hold the kernel's own begin and
 * end timestamps, and nothing is inserted into the stream around it. */
int gdg_profile_enable(gdg_ctx *ctx, int enable);
/* Bracket only every `every`-th process call (gdg_process_device / _window_device / host-buffer calls) while profiling is on: an event
 * pair costs a few microseconds AND keeps the bracketed kernel from overlapping its neighbours' ramp-up and tail, which is 5 % of a
 * 0.6 ms step when the dominant kernel of every step is bracketed.  1 = every call (default). */
int gdg_profile_sample(gdg_ctx *ctx, int every);
/* Drain the recorded pairs: total milliseconds and launch count of one kernel kind; resets it. */
int gdg_profile_read(gdg_ctx *ctx, int kind, double *total_ms, int *launches);

/* ---- tuner: tuner.Process / tuner.Analyze, one tuner per channel of the shard ------------------ */

typedef struct {
    double frequency;     /* tuner.Result.Frequency() */
    int32_t note_index;   /* index into the 61-note table (tuner/tuner.go:79-324), -1 = "Unknown" */
    int8_t cents;         /* tuner.Result.Cents() (truncated, tuner.go:557) */
} gdg_tuner_result;

/* tuner.Process for every channel: enqueue `frames` samples per channel into the 96000-sample rings. */
int gdg_tuner_enqueue(gdg_ctx *ctx, const double *const *samples, int frames, uint32_t sample_rate);
int gdg_tuner_enqueue_device(gdg_ctx *ctx, const double *d_samples, int frames, uint32_t sample_rate);
/* the same from the pinned INPUT slab of gdg_staging_buffers (row c = channel c): for hosts that may not hand over their own
 * pointers (the Go overlay of tuner.Tuner copies in[tunerChannel] into row 0 of a one-channel context) */
int gdg_tuner_enqueue_staged(gdg_ctx *ctx, int frames, uint32_t sample_rate);
/* One channel's whole ring at once: `n` must be the ring's length, 96000 (tuner/tuner.go:16 NUM_SAMPLES; anything else is GDG_ERR_INVALID),
 * samples oldest first -- what circular.Buffer.Retrieve hands out (tuner.go:392-399).  For a host that keeps the ring itself and only
 * analyses on the device (the Go overlay of tuner.Tuner: Process stays a host-side enqueue under the reference's lock): one upload per
 * analysis instead of twelve staged blocks.  Host buffer, blocks until it is consumed. */
int gdg_tuner_replace(gdg_ctx *ctx, int channel, const double *samples, int n, uint32_t sample_rate);
/* tuner.Analyze for every channel; results has n_channels entries.  Blocks. */
int gdg_tuner_analyze(gdg_ctx *ctx, gdg_tuner_result *results);
const char *gdg_tuner_note_name(int note_index);

/* ---- spatializer: partial N -> 2 mixdown of this shard ----------------------------------------- */

int gdg_spatializer_set_position(gdg_ctx *ctx, int channel, double azimuth, double distance, double level);
/* spatializer.SetSampleRate (rebuilds the history buffers; keeps the reference's 96000 quirk). */
int gdg_spatializer_set_sample_rate(gdg_ctx *ctx, uint32_t rate);
/*
 * spatializer.Process over the shard's channels WITHOUT the aux input: the host adds the
 * partial left/right pairs of all shards and then the aux buffer (spatializer.go:300-310).
 */
int gdg_spatialize(gdg_ctx *ctx, const double *const *in, double *out_left, double *out_right, int frames);
int gdg_spatialize_device(gdg_ctx *ctx, const double *d_in, double *d_out_lr, int frames);
/*
 * The same for hosts with the cgo pointer rules.  from_outputs == 0: the inputs are the rows of the pinned INPUT slab
 * (gdg_staging_buffers).  from_outputs != 0: the inputs are the chain outputs of the last gdg_process_staged, which are
 * still on the device -- controller.process() mixes exactly those (controller.go:2744-2761), so nothing is uploaded again.
 * out_left / out_right: `frames` float64 each, host memory.
 */
int gdg_spatialize_staged(gdg_ctx *ctx, int from_outputs, double *out_left, double *out_right, int frames);

/* ---- data formats either side of the path ---------------------------------------- */

/* wave/wave.go:51-60 sample formats x bit depths the reference reads and writes */
enum gdg_wave_format { GDG_FMT_LPCM8 = 0, GDG_FMT_LPCM16, GDG_FMT_LPCM24, GDG_FMT_LPCM32, GDG_FMT_IEEE32, GDG_FMT_IEEE64, GDG_FMT_COUNT };
int gdg_wave_bytes_per_sample(int format);      /* 0 for an unknown format */
/*
 * bytesToSamples + samplesToChannels (wave/wave.go:790-838, :237-270): the data section of a RIFF/WAVE file
 * (interleaved, little endian, `channels` x `samples_per_channel` samples) -> planar float64
 * [channels][samples_per_channel].  Bit exact with the reference.  Header parsing stays with the host.
 */
int gdg_wave_decode(gdg_ctx *ctx, int format, const void *bytes, size_t samples_per_channel, unsigned channels, double *samples);
int gdg_wave_decode_device(gdg_ctx *ctx, int format, const void *d_bytes, size_t samples_per_channel, unsigned channels, double *d_samples);
/* channelsToSamples + samplesToBytes (wave/wave.go:173-232, :737-785): the inverse, including the clipping rules. */
int gdg_wave_encode(gdg_ctx *ctx, int format, const double *samples, size_t samples_per_channel, unsigned channels, void *bytes);
int gdg_wave_encode_device(gdg_ctx *ctx, int format, const double *d_samples, size_t samples_per_channel, unsigned channels, void *d_bytes);

/* resample.Time (resample/resample.go:72-103): Lanczos-3 rate conversion; the length rule is :72-87. */
int gdg_resample_time_length(int input_length, uint32_t source_rate, uint32_t target_rate);
int gdg_resample_time(gdg_ctx *ctx, const double *samples, int n, uint32_t source_rate, uint32_t target_rate, double *out, int n_out);
int gdg_resample_time_device(gdg_ctx *ctx, const double *d_samples, int n, uint32_t source_rate, uint32_t target_rate, double *d_out, int n_out);

/*
 * level.Meter (level/level.go): n_ports independent channel meters (the reference runs 2N+3 of them:
 * inputs, outputs, master L/R, metronome).  gdg_meter_configure (re)creates them disabled and cleared;
 * process = level.go:147-210 for every enabled port over one buffer each; analyze = level.go:100-145
 * (integer dB, -200 floor).
 */
int gdg_meter_configure(gdg_ctx *ctx, int n_ports);
int gdg_meter_set_enabled(gdg_ctx *ctx, int port, int enabled);        /* port < 0: all ports (level.go:260-279) */
int gdg_meter_process(gdg_ctx *ctx, const double *const *buffers, int frames, uint32_t sample_rate);
int gdg_meter_process_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int frames, uint32_t sample_rate);
int gdg_meter_analyze(gdg_ctx *ctx, int32_t *levels, int32_t *peaks);
/* raw meter state of one port (current value, held peak, hold counter) for parity tests */
int gdg_meter_state(gdg_ctx *ctx, int port, double *current, double *peak, uint64_t *counter);

/*
 * metronome.Metronome (metronome/metronome.go): SetTick / SetTock (NULL = no sound), SetBeatsPerPeriod / SetSpeed /
 * SetSampleRate (none of them touches the counters, as in the reference), Process (:63-131) into one output buffer.
 */
int gdg_metronome_set_tick(gdg_ctx *ctx, const double *coefficients, int n);
int gdg_metronome_set_tock(gdg_ctx *ctx, const double *coefficients, int n);
int gdg_metronome_configure(gdg_ctx *ctx, uint32_t beats_per_period, uint32_t bpm_speed, uint32_t sample_rate);
int gdg_metronome_process(gdg_ctx *ctx, double *out, int frames);
int gdg_metronome_process_device(gdg_ctx *ctx, double *d_out, int frames);

/* ---- the batch run: controller.processFiles between "the files are read" and "the files are written" ------------- */

/*
 * One input of the batch run (controller/controller.go:2884-2990): the data section of a RIFF/WAVE file -- `channels` interleaved
 * channels of `samples_per_channel` samples in `format` -- of which channel `channel` feeds the input.  bytes == NULL or
 * samples_per_channel == 0 is the reference's "leaving channel empty" (silence; its rate does not matter).
 */
typedef struct {
    const void *bytes;
    size_t samples_per_channel;
    int format;                 /* enum gdg_wave_format */
    uint32_t sample_rate;
    unsigned channels, channel;
} gdg_batch_input;

typedef struct {
    uint32_t target_rate;       /* the session rate every input is resampled to (resample.Time, controller.go:2991-3003) */
    int out_format;             /* enum gdg_wave_format of the N + 3 outputs (the "lpcm" / "float" + bit depth prompts, :2821-2880) */
    int metronome_to_master;    /* metrMasterOutput: the metronome is the spatializer's aux input (:2744-2761) */
    int run_meters;             /* levelMeterEnabled: meters over the 2N + 3 ports configured with gdg_meter_configure (:2707-2781) */
    int tuner_enqueue;          /* != 0: every block also goes into the tuner rings (tuner.Process, :2668-2672) */
} gdg_batch_options;

/* samples of every output: the longest resampled input, rounded up to a multiple of BLOCK_SIZE = 8192 (controller.go:3005-3045) */
int gdg_batch_length(gdg_ctx *ctx, const gdg_batch_input *inputs, int n_inputs, uint32_t target_rate, size_t *samples);
/*
 * The whole batch on the device: decode -> resample.Time (inputs whose rate differs from the target) -> zero-pad -> for every
 * 8192-frame block: N x Chain.Process, metronome, spatializer (+ aux), meters -> encode.  n_inputs must equal the context's channel
 * count and max_frames must be >= 8192.  out_bytes: N + 3 host buffers (out_0 .. out_{N-1}, master_left, master_right, metronome,
 * controller.go:3123-3219; NULL = "skipping output") of gdg_batch_length() * gdg_wave_bytes_per_sample(out_format) bytes each.
 * Only file bytes cross PCIe: the samples stay in HBM from decode to encode.  Chains, spatializer positions, metronome and meters
 * are whatever was configured on the context; their state carries on from earlier calls, like the reference's.
 * The block loop runs in steps of up to gdg_ctx_set_window() blocks (a long run opens with a quarter and a half window, its tail
 * runs in halves down to one block: step sizes change the time blocking, never a sample).  The host side of the call -- gathering the
 * next steps' input bytes, scattering a finished step's output bytes -- runs beside the device on the calling thread, on the
 * context's copy workers (option copy_threads; two sets) and, for runs of more than three steps of four blocks or more, on ONE
 * helper thread that lives for the call; inputs and out_bytes are only read / written during the call.
 */
int gdg_batch_run(gdg_ctx *ctx, const gdg_batch_input *inputs, int n_inputs, const gdg_batch_options *options, void *const *out_bytes);
/*
 * The batch run of ONE SHARD of a job whose channels are split over several contexts / GPUs (contiguous channel blocks,
 * no collective).  The master mix is the sum over ALL channels, then the aux input, then the encoder's clip
 * (spatializer/spatializer.go:300-310, controller/controller.go:3123-3219); encoding a shard's partial mix would clip and truncate
 * before the sum.  So a shard hands out its partial sums as float64 and the caller finishes the master on any one context:
 *   for every shard g (in parallel, one context each):  gdg_batch_run_shard(ctx_g, inputs of g's channels, ..., out_bytes_g, &shard_g)
 *   then once:  gdg_batch_finish_master(ctx_0, fmt, {left_g}, {right_g}, G, aux, samples, rate, meters, master_left, master_right)
 * gdg_batch_run_shard = gdg_batch_run except: out_bytes holds the shard's n_inputs chain outputs only; master_left / master_right
 * receive gdg_batch_length() float64 samples each (this shard's channels mixed, NO aux, not clipped); the metronome runs on the
 * shard that passes metronome_bytes (its encoded track, the N + 3rd file) and / or metronome (the float64 track = the master's aux
 * input when metrMasterOutput is set) -- exactly one shard should; options->metronome_to_master must be 0 here (GDG_ERR_INVALID
 * otherwise: the aux input joins the master once, as `aux` of gdg_batch_finish_master); with run_meters the context carries 2 n + 3 ports of which a
 * shard feeds its inputs, its outputs and, if it runs it, the metronome.
 * gdg_batch_finish_master: master = ((p_0 + p_1) + ... + p_{G-1}) + aux per side, summed and encoded on ctx's device (aux may be
 * NULL; left_bytes / right_bytes NULL = "skipping output").  The shards' partial sums are associated differently from the single
 * context's sum over all channels (groups of 16 channels per shard, then shard order), so the sharded master equals gdg_batch_run's
 * to ~1e-16 relative, not bit for bit: a sample that sits on a 24- or 32-bit code boundary may come out one code apart.
 * run_meters != 0 feeds the two LAST ports of ctx's meters with the
 * finished master, block by block.
 */
typedef struct {
    double *master_left, *master_right;   /* host, gdg_batch_length() float64 each */
    void *metronome_bytes;                /* host, gdg_batch_length() encoded samples, or NULL */
    double *metronome;                    /* host, gdg_batch_length() float64, or NULL */
    size_t job_samples;                   /* samples of every output of the JOB (the longest gdg_batch_length over the shards: the
                                           * reference pads every channel to the longest input, controller.go:3005-3045); 0 = this
                                           * shard's own length */
} gdg_batch_shard_out;
int gdg_batch_run_shard(gdg_ctx *ctx, const gdg_batch_input *inputs, int n_inputs, const gdg_batch_options *options, void *const *out_bytes,
                        const gdg_batch_shard_out *shard);
int gdg_batch_finish_master(gdg_ctx *ctx, int out_format, const double *const *left, const double *const *right, int n_shards, const double *aux,
                            size_t samples, uint32_t sample_rate, int run_meters, void *left_bytes, void *right_bytes);
/*
 * The STREAMED batch run: the job of gdg_batch_run, fed and drained in slices of whole 8192-sample blocks.  Device and pinned memory
 * depend on the slice (one slice of decoded input, N x blocks x 8192 x 8 bytes) and on the context's window, not on the job's length,
 * and the outputs are byte for byte the one-call run's whatever the slicing: files of any length run in bounded memory, and the host
 * needs no more than one slice of every file resident.
 *   gdg_batch_stream_open(ctx, inputs, N, &options, &samples)          once; inputs[i].bytes is never read: NULL (or samples_per_channel
 *                                                                      == 0) still means "leaving channel empty", anything else "has
 *                                                                      samples"; samples_per_channel is the FILE's total (the RIFF header's)
 *   until `samples` are done:
 *     gdg_batch_stream_need(ctx, blocks, first, count)                 the source frames [first[i], first[i] + count[i]) of every input
 *                                                                      that the next slice of `blocks` blocks must bring (N entries each)
 *     gdg_batch_stream_step(ctx, blocks, in_bytes, out_bytes)          in_bytes[i]: those count[i] interleaved frames (all of the file's
 *                                                                      channels, the file's format; may be NULL when count[i] == 0);
 *                                                                      out_bytes: N + 3 buffers of blocks * 8192 * width bytes (NULL =
 *                                                                      "skipping output"), complete when the call returns
 *   gdg_batch_stream_close(ctx)                                        also before the end (an abandoned job); the context stays usable
 * `blocks` is any count from 1 to what is left of the job and may differ from slice to slice (one slice is at most 2^31 - 1 samples, the
 * job any size_t); inside a slice the block loop steps by the context's window as gdg_batch_run does, and the last slice carries the
 * job's zero padding.  first[i] continues exactly where the slice before ended: every source frame is handed over once, in order --
 * also frames no output sample reads -- and the few frames resample.Time looks back at are kept on the device.
 * Between open and close gdg_batch_run, gdg_batch_run_shard, gdg_batch_release and a second open return GDG_ERR_INVALID; so do step and
 * need without open, with `blocks` beyond the job's end, and after the last block.  A slice steps where the one-call run of the whole job
 * would step (or where the slice ends), so meters, tuner, metronome and the units' state are the one-call context's; a gdg_state_save
 * blob is equal as well where the job's last steps coincide (the convolution keeps two history halves, of which the one not read next
 * holds whatever frame the window grouping left there).  A slice that fails half-way closes the job (a checkpoint taken before it, below,
 * continues the job in a fresh context).  State
 * save / load and parameter changes between slices behave as between two gdg_batch_run calls.  The buffers are the batch run's own
 * (option stat_batch_device_kib reads their size, gdg_batch_release frees them).
 *
 * The streamed form of a SHARD (gdg_batch_run_shard / gdg_batch_finish_master in slices): a job split over several contexts / GPUs whose
 * files are too long to hold.  Per shard g, one context each:
 *   gdg_batch_stream_open_shard(ctx_g, inputs of g's channels, n, &options, job_samples, run_metronome, &samples)
 *                                                                      gdg_batch_stream_open under gdg_batch_run_shard's rules:
 *                                                                      options->metronome_to_master must be 0; job_samples = the job's
 *                                                                      length (the longest gdg_batch_length over the shards, a multiple
 *                                                                      of 8192 and not shorter than the shard's own; 0 = the shard's own),
 *                                                                      returned in `samples` -- the shard pads to it; run_metronome says
 *                                                                      ONCE, for the whole job, whether this shard runs the metronome
 *                                                                      (exactly one shard should); with run_meters the context carries
 *                                                                      2 n + 3 ports, fed as gdg_batch_run_shard feeds them
 *   per slice: gdg_batch_stream_need as above, then
 *     gdg_batch_stream_step_shard(ctx_g, blocks, in_bytes, out_bytes, &slice)
 *                                                                      out_bytes: the shard's n chain outputs of blocks * 8192 * width
 *                                                                      bytes (NULL = "skipping output"); slice.master_left / master_right
 *                                                                      (required) receive blocks * 8192 float64 each: this shard's partial
 *                                                                      mix of the slice, no aux, not clipped; slice.metronome_bytes /
 *                                                                      slice.metronome (either may be NULL in any slice) the slice's
 *                                                                      encoded / float64 metronome track -- GDG_ERR_INVALID when the job
 *                                                                      was opened with run_metronome == 0; slice.job_samples is ignored
 *   gdg_batch_stream_close(ctx_g)
 * and once per slice, when every shard has delivered it:
 *   gdg_batch_finish_master_slice(ctx, fmt, {left_g}, {right_g}, G, aux, blocks * 8192, rate, meters, left_bytes, right_bytes)
 *                                                                      the arguments, the result and the bits of gdg_batch_finish_master
 *                                                                      for a whole number of blocks (GDG_ERR_INVALID otherwise) -- the
 *                                                                      same code path, made for the job's critical path: the partials
 *                                                                      gathered into one pinned slab, one upload, one kernel and one
 *                                                                      download per piece
 * A shard's slices step where the ONE-CALL gdg_batch_run_shard of the whole job would step, so chain outputs, partial sums, metronome,
 * meters, tuner and unit state are that run's whatever the slicing, and the finished slices put together are gdg_batch_finish_master's
 * bytes.  gdg_batch_stream_step on a job opened as a shard and gdg_batch_stream_step_shard on a job opened with gdg_batch_stream_open
 * return GDG_ERR_INVALID and write nothing; every other rule of the streamed run above holds for a shard's job as well.
 * A context runs ONE call at a time.  Any context may finish slice s (its last two meter ports receive the master when asked); a caller
 * who wants the finish of slice s to run beside shard 0's slice s + 1 gives the finish a context of its own.
 *
 * gdg_batch_stream_span is pure arithmetic and needs no context or device: the source frames of one input that the job's output samples
 * [out_first, out_first + out_count) read, for an input of samples_per_channel frames at source_rate in a job at target_rate.  Same
 * rate: the range itself, cut at the file's end.  Otherwise the hull of the resampler's windows floor(i dx) - 2 .. floor(i dx) + 3,
 * dx = source_rate / target_rate (resample/resample.go:88-103), over the samples the input covers (resample.go:72-87), cut to
 * [0, samples_per_channel).  A range that reads nothing gives src_count = 0 (src_first = samples_per_channel).
 */
int gdg_batch_stream_span(size_t samples_per_channel, uint32_t source_rate, uint32_t target_rate, size_t out_first, size_t out_count,
                          size_t *src_first, size_t *src_count);
int gdg_batch_stream_open(gdg_ctx *ctx, const gdg_batch_input *inputs, int n_inputs, const gdg_batch_options *options, size_t *samples);
int gdg_batch_stream_need(gdg_ctx *ctx, int blocks, size_t *first, size_t *count);
int gdg_batch_stream_step(gdg_ctx *ctx, int blocks, const void *const *in_bytes, void *const *out_bytes);
int gdg_batch_stream_close(gdg_ctx *ctx);
int gdg_batch_stream_open_shard(gdg_ctx *ctx, const gdg_batch_input *inputs, int n_inputs, const gdg_batch_options *options, size_t job_samples,
                                int run_metronome, size_t *samples);
int gdg_batch_stream_step_shard(gdg_ctx *ctx, int blocks, const void *const *in_bytes, void *const *out_bytes, const gdg_batch_shard_out *slice);
int gdg_batch_finish_master_slice(gdg_ctx *ctx, int out_format, const double *const *left, const double *const *right, int n_shards, const double *aux,
                                  size_t samples, uint32_t sample_rate, int run_meters, void *left_bytes, void *right_bytes);
/*
 * CHECKPOINT of a streamed batch run: no reference counterpart.  One blob that holds everything a streamed job (plain or a shard's)
 * carries from one slice to the next, written between any two slices -- also before the first and after the last -- and loaded into a
 * new process, context or device, where the job continues with the bytes the uninterrupted run would have written:
 *   gdg_batch_stream_checkpoint_size(ctx, &bytes); gdg_batch_stream_checkpoint(ctx, blob, capacity, &written)
 *                                                                      valid between open and close; ordered after everything queued
 *                                                                      on the context; NO side effects (gdg_state_save's contract: the
 *                                                                      sums made ahead are kept, a job with a checkpoint between every
 *                                                                      two slices writes the same bytes as one without); into less
 *                                                                      capacity it fails with *written = the size needed
 *   gdg_batch_stream_resume(ctx, inputs, N, &options, blob, bytes, &samples_done)
 *   gdg_batch_stream_resume_shard(ctx, inputs, n, &options, job_samples, run_metronome, blob, bytes, &samples_done)
 *                                                                      in the place of gdg_batch_stream_open / _open_shard on a context
 *                                                                      with no job open; on success the job is open at the recorded
 *                                                                      position (*samples_done), gdg_batch_stream_need continues first[i]
 *                                                                      where the checkpointed job stood, and a blob taken after the last
 *                                                                      block gives a job that has delivered its last block
 * STATE, in the blob: the job (position, length, per input the frames handed over and the samples it covers, the inputs' metadata, the
 * options, for a shard `shard`, run_metronome and job_samples); the gdg_state_save blob of all channels, unchanged (version 1); per
 * resampled input the GDG_STREAM_CARRY = 8 source frames resample.Time looks back at and how many of them are valid; per meter port
 * value, held peak and hold counter; the tuner rings (oldest sample first) with their rate, present when the source had rings; the
 * metronome's sample and tick counters.  CONFIGURATION, with the target: chains, parameters, filter taps, spatializer positions,
 * metronome sounds and settings, gdg_meter_configure and the ports' enabled flags, window (gdg_ctx_set_window) and channel groups --
 * the caller sets the target up as for a fresh job; window and groups may differ from the source's (a delay line is rotated into the
 * target's ring and windows give the bits of single frames, so the continued bytes depend on neither).
 * inputs and options are given again (the blob holds no pointers) and checked against the recorded job: channel count; per input
 * has-samples, samples_per_channel, format, rate, channels, channel; target_rate, out_format, the three flags; a shard's job_samples and
 * run_metronome; a shard's blob is refused by gdg_batch_stream_resume and a plain one by _resume_shard.  A resume is ALL OR NOTHING, in
 * this order: the digest; the job; every layout key of the embedded channel state (as gdg_state_load); meter port count and tuner ring
 * length; only then it writes.  A mismatch returns GDG_ERR_INVALID with gdg_last_error naming what did not fit, writes nothing and
 * leaves no job open.
 * Container (opaque; little-endian, stable within one version): a 48-byte header {"GDGCKPT\0", version 1, payload offset = 48, total
 * bytes, reserved, 16 bytes of digest}, then the payload -- a directory of six sections {offset, bytes} (job, channel state, meters,
 * tuner, metronome, resampler carry; bytes 0 = absent) and the sections at 16-byte alignment.
 * DIGEST, over the payload bytes [48, total) cut into n granules of 16 bytes, granule g = two little-endian 64-bit words a_g, b_g; all
 * arithmetic modulo 2^64, K = 0x9e3779b97f4a7c15, M0 = 0xff51afd7ed558ccd, M1 = 0xc4ceb9fe1a85ec53:
 *   u_g = t ^ (t >> 32) with t = (a_g + (g + 1) K) M0;     v_g = s ^ (s >> 29) with s = (b_g ^ u_g) M1
 *   S0 = sum of u_g;  S1 = XOR of v_g;     fmix(x): x ^= x >> 33, x *= M0, x ^= x >> 33, x *= M1, x ^= x >> 33
 *   D0 = fmix(S0 + K + n);  D1 = fmix(S1 ^ D0);     stored as D0, D1 little-endian
 * Order-sensitive (g enters every term) and independent of how the device splits the work (sum and XOR commute).  It is taken on the
 * device: over the staged blob just gathered in a checkpoint, over the uploaded copy before anything else in a resume.  The digest is
 * for INTEGRITY ONLY -- truncation, bit rot, a torn write; it is no authentication and no defence against a crafted blob.
 * gdg_state_verify checks a container's digest (on ctx's device) and writes nothing; a bare gdg_state_save blob carries no digest and
 * is GDG_ERR_INVALID, saying so.
 */
int gdg_batch_stream_checkpoint_size(gdg_ctx *ctx, size_t *bytes);
int gdg_batch_stream_checkpoint(gdg_ctx *ctx, void *blob, size_t capacity, size_t *written);
int gdg_batch_stream_resume(gdg_ctx *ctx, const gdg_batch_input *inputs, int n_inputs, const gdg_batch_options *options, const void *blob,
                            size_t bytes, size_t *samples_done);
int gdg_batch_stream_resume_shard(gdg_ctx *ctx, const gdg_batch_input *inputs, int n_inputs, const gdg_batch_options *options, size_t job_samples,
                                  int run_metronome, const void *blob, size_t bytes, size_t *samples_done);
int gdg_state_verify(gdg_ctx *ctx, const void *blob, size_t bytes);
/* The device buffers of a batch run (the decoded inputs are the large part: N x length x 8 bytes) stay with the context for the next
 * run of the same or a smaller size; this frees them. */
int gdg_batch_release(gdg_ctx *ctx);
/*
 * RENDER REPORT: no reference counterpart.  What a batch call rendered, per output port and per block of 8192 samples, taken on the
 * device from the float64 rows just before the encoder reads them (filter.Process clamps every power amp to +-1 and the encoder clamps
 * again before it quantises; neither says so).  One record per (port, block):
 */
typedef struct {
    double   peak;        /* max |x| over the block's finite samples; 0 when there is none */
    double   sum_sq;      /* sum of x*x over the block's finite samples */
    uint32_t peak_index;  /* first index inside the block with |x| == peak; 0 when peak == 0 */
    uint32_t clipped;     /* samples with |x| > 1: the ones the encoder's clamp changes */
    uint32_t full_scale;  /* samples with |x| >= 1 (a power amp's clamp leaves exactly +-1) */
    uint32_t nonfinite;   /* NaN, +inf, -inf: counted, and left out of the four fields above */
} gdg_block_stats;        /* 32 bytes, little-endian, no padding */
/*
 * The statistics of a block are stateless.  sum_sq is added in an order that depends on the block's LENGTH and on nothing else -- not on
 * the row, the row count, the block's place in the buffer, the window, the slicing or the sharding -- with every square and every add
 * rounded on its own (no fused multiply-add): the same samples give the same 64 bits wherever they sit.  A tie on the peak goes to the
 * lower index.
 *   gdg_block_stats_rows(ctx, rows, n_rows, samples, block, records)   n_rows host rows of `samples` float64 each, cut into blocks of
 *                                                                      `block` >= 1 samples (the last one of a row may be short);
 *                                                                      records: [n_rows][ceil(samples / block)], row-major
 *   gdg_block_stats_rows_device(ctx, d_rows, row_stride, n_rows, samples, block, d_records)
 *                                                                      the same on device memory, enqueued on gdg_ctx_stream: row r
 *                                                                      at d_rows + r * row_stride (row_stride >= samples, any 8-byte
 *                                                                      alignment); no sample outside [row, row + samples) is read
 *   gdg_batch_report_enable(ctx, enable)                               from the next batch call on, every batch call of the context
 *                                                                      keeps the records of what it rendered (blocks of 8192).
 *                                                                      Configuration, like the window: not part of a checkpoint
 *                                                                      (the container stays version 1) -- set it again on the target
 *                                                                      of a resume.  Off (the default): no launch, allocation or
 *                                                                      byte differs from a context that never heard of it
 *   gdg_batch_report(ctx, records, capacity, &ports, &blocks)          the records of the LAST COMPLETED batch call of the context,
 *                                                                      [ports][blocks] row-major; records == NULL: the two counts
 *                                                                      only.  GDG_ERR_INVALID (gdg_last_error says which) when
 *                                                                      capacity < ports * blocks, or when there is no report: none
 *                                                                      was enabled before the call ran, or no call has completed
 * Ports, in this order:
 *   gdg_batch_run, gdg_batch_stream_step                   the N chain outputs, master left, master right, metronome -- the order of
 *                                                          out_bytes, the master after the aux add; a NULL in out_bytes changes nothing
 *   gdg_batch_run_shard, gdg_batch_stream_step_shard       the n chain outputs, then the metronome (all-zero records on a shard that
 *                                                          does not run it); the partial master is not a port
 *   gdg_batch_finish_master, gdg_batch_finish_master_slice master left, master right: the sums after the aux add, before the clamp
 * The records come down with each step's own download; a slice's report covers the slice's blocks.
 */
int gdg_block_stats_rows(gdg_ctx *ctx, const double *const *rows, int n_rows, size_t samples, int block, gdg_block_stats *records);
int gdg_block_stats_rows_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, int block,
                                gdg_block_stats *d_records);
int gdg_batch_report_enable(gdg_ctx *ctx, int enable);
int gdg_batch_report(gdg_ctx *ctx, gdg_block_stats *records, size_t capacity, int *ports, size_t *blocks);
/*
 * BAND SPECTRUM: no reference counterpart.  What a block of the render report sounds like: the power of every block of 8192 samples in up
 * to 32 frequency bands, from the same float64 rows, on the device.  Stateless like the record beside it: a block's bands are a function
 * of that block's samples (and of the rate and the edges) and of nothing else.  The quantity, for block j of a row at sample rate R, with
 * L = 8192 samples x[n] (a non-finite sample is taken as 0 -- gdg_block_stats.nonfinite counts them; a short last block is zero-padded):
 *   window     w[n] = 0.5 - 0.5 cos(2 pi n / L)                          (periodic Hann)
 *   transform  X[k] = sum_n w[n] x[n] exp(-2 pi i k n / L),              k = 0 .. L/2
 *   bin power  P[k] = c_k |X[k]|^2 / (L^2 * 3/8),                        c_0 = c_{L/2} = 1, c_k = 2 otherwise
 *   bands      n_edges edges in Hz, 2 <= n_edges <= 33, finite, >= 0, strictly ascending: n_edges - 1 bands, at most 32;
 *              k_lo[b] = clamp((long long)ceil(edges[b] * 8192.0 / R), 0, 4097), computed on the host in float64 as written;
 *              band b = the sum of P[k] over k_lo[b] <= k < k_lo[b + 1]
 * Known answers: by Parseval the sum of P[k] over all bins is sum((w x)^2) / (L * 3/8), the block's mean square; a bin-centred sine of
 * amplitude A puts A^2/3 into its own bin and A^2/12 into each neighbour, A^2/2 in all (a sine of amplitude 0.5 at bin 100: 0.25/12,
 * 0.25/3, 0.25/12 in bins 99, 100, 101).  A band that holds no bin -- edges above Nyquist, two edges inside one bin -- is exactly 0.0, and
 * so is every band of an all-zero block.
 * The sums are added in an order that depends on L and the bin ranges alone -- not on the row, the row count, the grid, the block's place,
 * the window, the slicing or the sharding -- with every square and every add rounded on its own, and without atomics: the same samples
 * give the same 64 bits wherever they sit.
 *   gdg_block_spectrum_rows(ctx, rows, n_rows, samples, sample_rate, edges_hz, n_edges, bands)
 *                                                                      n_rows host rows of `samples` float64 each;
 *                                                                      bands: [n_rows][ceil(samples / 8192)][n_edges - 1], row-major
 *   gdg_block_spectrum_rows_device(ctx, d_rows, row_stride, n_rows, samples, sample_rate, edges_hz, n_edges, d_bands)
 *                                                                      the same on device memory, enqueued on gdg_ctx_stream: row r
 *                                                                      at d_rows + r * row_stride (row_stride >= samples, any 8-byte
 *                                                                      alignment); no sample outside [row, row + samples) is read.
 *                                                                      edges_hz is host memory
 *   gdg_batch_spectrum_enable(ctx, edges_hz, n_edges)                  from the next batch call on, every batch call of the context
 *                                                                      keeps the bands of what it rendered.  n_edges == 0: off (the
 *                                                                      default: no launch, allocation, upload or byte differs from a
 *                                                                      context that never heard of it).  The list is validated whole
 *                                                                      before it replaces the one in force.  Configuration, like
 *                                                                      gdg_batch_report_enable, the source map and the dither: part
 *                                                                      of no blob (the checkpoint container stays version 1) -- set
 *                                                                      it again on the target of a resume -- and GDG_ERR_INVALID
 *                                                                      while a streamed job is open.  R is the job's target_rate;
 *                                                                      the two finish calls use their sample_rate argument (which
 *                                                                      must then be positive)
 *   gdg_batch_spectrum(ctx, bands, capacity, &ports, &blocks, &n_bands) the bands of the LAST COMPLETED batch call of the context,
 *                                                                      [ports][blocks][n_bands] row-major; bands == NULL: the three
 *                                                                      counts only.  GDG_ERR_INVALID when capacity < ports * blocks
 *                                                                      * n_bands (the three counts are filled in), or when there
 *                                                                      is no spectrum
 * Ports and their order are the render report's, call by call (above); the report and the spectrum are independent switches.  The bands
 * come down with each step's own download, behind the records; a slice's spectrum covers the slice's blocks.
 */
int gdg_block_spectrum_rows(gdg_ctx *ctx, const double *const *rows, int n_rows, size_t samples, uint32_t sample_rate, const double *edges_hz,
                            int n_edges, double *bands);
int gdg_block_spectrum_rows_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, uint32_t sample_rate,
                                   const double *edges_hz, int n_edges, double *d_bands);
int gdg_batch_spectrum_enable(gdg_ctx *ctx, const double *edges_hz, int n_edges);
int gdg_batch_spectrum(gdg_ctx *ctx, double *bands, size_t capacity, int *ports, size_t *blocks, int *n_bands);
/*
 * ALIGNMENT: no reference counterpart.  When a block of one output arrives relative to the same block of another, and with which polarity:
 * the first question when two renders of one take are blended or summed (a few samples of offset comb-filter the sum, an inverted rig
 * cancels).  From the same float64 rows, on the device; stateless like the record and the bands: a function of the two blocks and M.
 * L = 8192.  A call has `ports` rows; port p has a reference ref[p]: -1 (not measured) or a port of the same call (ref[p] == p is
 * allowed).  M = max_lag, 1 <= M <= 2048.  For block b, x = the block of row ref[p], y = the block of row p, NaN and +-inf taken as 0, a
 * short last block zero-padded to L:
 *   r[l] = sum_{n = M}^{L-M-1} x[n] * y[n + l]                          for -M <= l <= M
 * The central L - 2M samples of the reference against the whole block of p: every product lies inside the block for every lag, so this is
 * a linear correlation without wrap-around and without edge weighting.  A positive lag: p arrives LATER than its reference.
 */
typedef struct {
    double   corr;        /* r[lag], signed: negative = opposite polarity */
    double   corr0;       /* r[0]: what the pair has without a shift */
    double   ref_sq;      /* sum_{n=M}^{L-M-1} x[n]^2 */
    double   sq_at_lag;   /* sum_{n=M}^{L-M-1} y[n + lag]^2; corr / sqrt(ref_sq * sq_at_lag) is the normalised coefficient in [-1, 1] */
    int32_t  lag;         /* the l with the greatest |r[l]| as computed on the device; equal magnitudes: the smaller |l|, then the negative one */
    uint32_t reserved;    /* 0 */
} gdg_block_align;        /* 40 bytes, little-endian, no padding other than the last field */
/*
 * r is computed by transform (one 8192-point complex transform of x' + i y, x' = x zeroed outside [M, L - M), and one inverse), so corr and
 * corr0 carry the transform's rounding: a few 1e-16 of (ref_sq + sum y^2), which is of the order of sqrt(ref_sq * sum y^2) when the two
 * rows are of one size and more than that when one is much the quieter.  The choice among equal magnitudes is made lexicographically at every level of a fixed reduction tree, so `lag` is a function
 * of the two blocks and M alone; ref_sq and sq_at_lag are added in an order that depends on M (and lag) alone, every square and add rounded
 * on its own, without atomics: the same samples give the same bits whatever the row, the grid, the window, the slicing or the sharding.
 * A port with ref[p] = -1 gets an all-zero record; two silent blocks give lag = 0 and zeros everywhere.
 *   gdg_block_align_rows(ctx, rows, n_rows, samples, ref, max_lag, records)
 *                                                                      n_rows host rows of `samples` float64 each, ref: n_rows
 *                                                                      entries; records: [n_rows][ceil(samples / 8192)], row-major
 *   gdg_block_align_rows_device(ctx, d_rows, row_stride, n_rows, samples, ref, max_lag, d_records)
 *                                                                      the same on device memory, enqueued on gdg_ctx_stream: row r
 *                                                                      at d_rows + r * row_stride (row_stride >= samples, any 8-byte
 *                                                                      alignment); no sample outside [row, row + samples) is read.
 *                                                                      ref is host memory; d_records (8-byte aligned) gets the
 *                                                                      records of the measured rows, the others are zeroed
 *   gdg_batch_align_enable(ctx, ref, n_ports, max_lag)                 from the next batch call on, every batch call of the context
 *                                                                      keeps the alignment records of what it rendered.  ref == NULL
 *                                                                      or n_ports == 0: off (the default: no launch, allocation,
 *                                                                      upload or byte differs).  The list is validated whole before
 *                                                                      it replaces the one in force.  n_ports is the port count of
 *                                                                      the calls to come -- N + 3 for gdg_batch_run and
 *                                                                      gdg_batch_stream_step, n + 1 for the shard forms -- and a
 *                                                                      batch call with another count is refused before it does
 *                                                                      anything.  Configuration, like gdg_batch_spectrum_enable:
 *                                                                      part of no blob -- set it again on the target of a resume --
 *                                                                      and GDG_ERR_INVALID while a streamed job is open
 *   gdg_batch_align(ctx, records, capacity, &ports, &blocks)           the records of the LAST COMPLETED batch call of the context,
 *                                                                      [ports][blocks] row-major; records == NULL: the two counts
 *                                                                      only.  GDG_ERR_INVALID when capacity < ports * blocks (the
 *                                                                      counts are filled in), or when there are no records
 * Ports and their order are the render report's.  The two finish calls carry no alignment records (after one, there are none): a
 * reference is a port of the same call, and the master's two sides are one mix.  On a shard that does not run the metronome, a record that
 * measures or references the metronome port is all-zero.  The records come down with each step's own download, behind the bands; report,
 * spectrum and alignment are independent switches.
 */
int gdg_block_align_rows(gdg_ctx *ctx, const double *const *rows, int n_rows, size_t samples, const int *ref, int max_lag, gdg_block_align *records);
int gdg_block_align_rows_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, const int *ref, int max_lag,
                                gdg_block_align *d_records);
int gdg_batch_align_enable(gdg_ctx *ctx, const int *ref, int n_ports, int max_lag);
int gdg_batch_align(gdg_ctx *ctx, gdg_block_align *records, size_t capacity, int *ports, size_t *blocks);
/*
 * TRUE PEAK: no reference counterpart.  gdg_block_stats.peak is the largest SAMPLE; it cannot see the waveform between the samples.  A sine
 * at a quarter of the sample rate whose samples fall 45 degrees off its crests reads peak = 0.707 A, and every DAC, sample-rate converter
 * and lossy encoder downstream reconstructs A.  The true-peak record is the largest magnitude of the block 4x oversampled: its samples and
 * the three points a 24-tap windowed-sinc interpolator puts between two of them.  From the same float64 rows, on the device; stateless
 * like the record, the bands and the alignment record: a function of the block's samples and of nothing else.
 * Block length L = 8192, oversampling factor 4, half-width H = 12.  A non-finite sample is taken as 0.  A short last block is just
 * shorter (length l); it is not padded.
 * Taps, for phase p = 1, 2, 3 and j = -H+1 .. H (24 per phase), with t = p/4 - j:
 *   g_p[j] = sinc(t) * (0.5 + 0.5 cos(pi t / H)),  sinc(t) = sin(pi t) / (pi t);   h_p[j] = g_p[j] / sum_j g_p[j]
 * built in float64 on the host, once (csrc/true_peak_taps.h), the normalising sum added in ascending j.  Each phase sums to 1: DC is exact.
 * Interpolated points, for every n with H-1 <= n <= l-H-1:
 *   v_p[n] = sum_j x[n + j] * h_p[j]                                    the value at position n + p/4
 * accumulated from 0.0 in ascending j, every product and every add rounded on its own (no fused multiply-add, no use of the taps'
 * symmetry).  Only points whose 24 samples all lie inside the block are evaluated: in each block the 11 sample intervals at either end
 * are not looked at, and neither is the interval that crosses into the next block -- 23 intervals per block boundary, 0.28 % of the
 * stream.  That is the price of statelessness, the price the alignment record pays with its central slice.  A block with l < 24 has no
 * interpolated point.
 */
typedef struct {
    double   true_peak;   /* max of |x[n]| over all l samples and of |v_p[n]| over all evaluated points; never below gdg_block_stats.peak; 0 for a silent block */
    uint32_t position;    /* 4 n + p (p = 0 for a sample) of the FIRST point that attains it: a tie goes to the lower position; 0 when true_peak == 0 */
    uint32_t overs;       /* interpolated points (p != 0) with |v| > 1; the samples' own overs are gdg_block_stats.clipped */
} gdg_block_true_peak;    /* 16 bytes, little-endian, no padding */
/*
 * A value is a fixed-order sum over 24 samples and max is exact, so the record's 16 bytes are a function of the block's samples alone: not
 * of the row, the grid, the block's place, the window, the slice or the shard.  Known answers (L = 8192):
 *   an impulse of 1.0 at sample 4000                    true_peak 1.0, position 16000, overs 0; its two half-way neighbours read 0.633825
 *   a constant 0.5                                      true_peak in [0.5, 0.5 (1 + 24 * 2^-52)], overs 0
 *   0.9 sin(2 pi n / 4 + pi / 4)                        sample peak 0.636396, true_peak 0.900330 (the p = 2 gain at fs/4 is 1.000366),
 *                                                       position = 2 (mod 4)
 *   the gain of the three phases                        within 5e-4 of 1 up to 0.25 fs and within 1.5e-3 up to 0.35 fs (the worst, p = 2: +1.46e-3
 *                                                       at fs/3), +0.5 % (p = 2) at 0.4 fs, -10 % (p = 2) at 0.45 fs
 *   gdg_true_peak_taps(taps, capacity)                                 the library's table into taps[3][24] (phase 1, 2, 3; j ascending).
 *                                                                      No context, no device.  GDG_ERR_INVALID when taps is NULL or
 *                                                                      capacity < 72
 *   gdg_block_true_peak_rows(ctx, rows, n_rows, samples, records)      n_rows >= 1 host rows of `samples` float64 each, in blocks of
 *                                                                      8192 (the last of a row may be short); records:
 *                                                                      [n_rows][ceil(samples / 8192)], row-major
 *   gdg_block_true_peak_rows_device(ctx, d_rows, row_stride, n_rows, samples, d_records)
 *                                                                      the same on device memory, enqueued on gdg_ctx_stream: row r
 *                                                                      at d_rows + r * row_stride (row_stride >= samples, any 8-byte
 *                                                                      alignment); no sample outside [row, row + samples) is read;
 *                                                                      d_records is 8-byte aligned
 *   gdg_batch_true_peak_enable(ctx, enable)                            from the next batch call on, every batch call of the context
 *                                                                      keeps the true-peak records of what it rendered.  Off (the
 *                                                                      default): no launch, allocation, upload or byte differs.
 *                                                                      Configuration, like gdg_batch_report_enable: part of no blob
 *                                                                      -- set it again on the target of a resume -- and
 *                                                                      GDG_ERR_INVALID while a streamed job is open
 *   gdg_batch_true_peak(ctx, records, capacity, &ports, &blocks)       the records of the LAST COMPLETED batch call of the context,
 *                                                                      [ports][blocks] row-major; records == NULL: the two counts
 *                                                                      only.  GDG_ERR_INVALID when capacity < ports * blocks (the
 *                                                                      counts are filled in), or when there are no records
 * Ports and their order are the render report's, call by call, the two finish calls included: they measure the sums the record measures
 * (after the aux, before the encoder's clamp).  The rows are read before the dither.  The records come down with each step's own download,
 * behind the alignment records; report, spectrum, alignment and true peak are independent switches.
 */
int gdg_true_peak_taps(double *taps, int capacity);
int gdg_block_true_peak_rows(gdg_ctx *ctx, const double *const *rows, int n_rows, size_t samples, gdg_block_true_peak *records);
int gdg_block_true_peak_rows_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, gdg_block_true_peak *d_records);
int gdg_batch_true_peak_enable(gdg_ctx *ctx, int enable);
int gdg_batch_true_peak(gdg_ctx *ctx, gdg_block_true_peak *records, size_t capacity, int *ports, size_t *blocks);
/*
 * SHARED SOURCES: no reference counterpart.  Re-amping renders one take, or a handful, through hundreds of rigs: with a source map every
 * shared input is gathered, uploaded, decoded and (when its rate is not the job's) resampled ONCE and stored to the row of every channel
 * that reads it, instead of once per channel.
 *   gdg_batch_set_sources(ctx, source, n)                              source[c] = the channel whose input entry channel c reads.
 *                                                                      source[c] == c: the channel reads its own entry (a ROOT; what
 *                                                                      every channel does without a map).  Anything else makes c a
 *                                                                      READER, and source[c] must be a root: source[source[c]] ==
 *                                                                      source[c].  n = the context's channel count.  source == NULL
 *                                                                      or n == 0 clears the map.
 * Configuration, like the window and gdg_batch_report_enable: it holds from the next batch call on, survives batch calls and is part of
 * no blob.  A malformed map -- an entry out of range, a reader of a reader, the wrong n -- is GDG_ERR_INVALID, gdg_last_error names the
 * offending channel, and the map in force stays in force; so does a call while a streamed job is open.
 * With a map in force, in gdg_batch_run, gdg_batch_run_shard, gdg_batch_stream_open and gdg_batch_stream_open_shard:
 *   n_inputs stays the channel count.  inputs[c] of a reader is never looked at: the reader takes the metadata, the length, the
 *   empty-or-not status and the samples of its root (a reader of an empty root is silent).
 *   gdg_batch_length is unchanged: it looks at every entry it is given and knows no map.  The engine computes the job's length over
 *   the ROOTS; a caller that sizes its buffers with gdg_batch_length leaves the readers' entries empty (or copies of their roots').
 *   gdg_batch_stream_need reports count[c] == 0 for a reader and first[c] = its root's first; in_bytes[c] of a reader is never read
 *   and may be NULL.
 *   Everything downstream is byte for byte that of the same job without a map whose readers' entries are copies of their roots': the
 *   N + 3 files, a shard's partial master and metronome, the meters over the 2 N + 3 ports, the tuner rings, the render report, and the
 *   units' state as an equal gdg_state_save blob.  A reader's row gets the bits the per-channel decoder and resampler give.
 *   A map spans one context: a reader and its root live on the same shard.
 * LIMIT: a job with shared sources cannot be checkpointed yet.  While the map in force has at least one reader,
 * gdg_batch_stream_checkpoint, gdg_batch_stream_checkpoint_size, gdg_batch_stream_resume and gdg_batch_stream_resume_shard return
 * GDG_ERR_UNSUPPORTED (the version-1 container records positions and resampler carries per input).  No map, or a map without a reader,
 * checkpoints exactly as before.
 * Off -- no map, or every channel its own root -- no launch, allocation, upload or byte differs from a context that never heard of the
 * call.  Options stat_batch_upload_bytes and stat_batch_resampled_samples read what the last call moved and resampled.
 */
int gdg_batch_set_sources(gdg_ctx *ctx, const int *source, int n);
/*
 * DITHER: no reference counterpart.  samplesToBytes (and gdg_wave_encode, which restates it) scales and TRUNCATES TOWARD ZERO: the zero code
 * is two steps wide, everything below one code vanishes, and the error follows the signal.  With dither in force the four LPCM formats of
 * a batch call are written with TPDF dither and rounding instead; IEEE32 and IEEE64 outputs are never dithered and keep their bytes.
 * The noise of a sample depends on (seed, port, absolute sample index) alone, so a file comes out byte for byte the same whatever the
 * window, the slicing, the sharding, a checkpoint / resume in between or a source map.  All integer arithmetic modulo 2^64; K, M0, M1 and
 * fmix are the checkpoint digest's (above):
 *   key = fmix(seed + (port + 1) K)                once per row
 *   h   = fmix((index + K) ^ key)                  index: 64-bit sample index within the job, 0 = first sample of the file
 *   a   = h >> 32,  b = h & 0xffffffff
 *   d   = (double)((int64)a - (int64)b) * 2^-32    triangular on (-1, 1) codes; exact in float64
 *   t   = S * clamp1(x)                            S = 127, 32767.5, 8388607.5, 2147483647.5: the plain encoder's constants
 *   q   = floor((t + d) + 0.5)                     the product and the two adds each rounded on their own (no fused multiply-add)
 *   code = clamp(q, the format's range)            LPCM8: + 128 afterwards, clamped to 0 .. 255
 * Known answers (seed, port, index, x -> h, LPCM16 code, LPCM24 code):
 *   0x0, 0, 0, 0.0 -> 0xdf9545e13007448a, 1, 1          0x63, 3, 8192, 1e-5 -> 0x33a34e84d34b5c4b, 0, 83
 *   0x3039, 7, 0x100000000, -0.7 -> 0xe8f8277b0aa97796, -22936, -5872024
 * NaN and infinities: whatever the conversion gives; not specified.
 * PORTS: chain output c of a context is port port_base + c, port_base = the job-wide index of the context's first channel (0 for an
 * unsharded job).  The job-wide outputs have fixed ports, so a shard need not know the job's channel count: master left 0xfffffffd,
 * master right 0xfffffffe, metronome 0xffffffff.  port_base + the context's channel count stays below 0xfffffffd.
 * INDEX: a sample's position in the job.  gdg_batch_run and gdg_batch_run_shard start at 0; a slice of a streamed job starts at the job's
 * position, which gdg_batch_stream_resume and _resume_shard restore.  gdg_batch_finish_master starts at 0 and leaves the master cursor
 * alone; gdg_batch_finish_master_slice starts at the context's master cursor and, when it returns GDG_OK, advances it by its `samples`.
 *   gdg_batch_set_dither(ctx, mode, seed, port_base)   mode 0 = off, 1 = TPDF as above; anything else is GDG_ERR_INVALID (gdg_last_error
 *                                                      says so) and the setting in force stays; so does a port_base out of range (mode 1), and
 *                                                      a call while a streamed job is open.  Resets the master cursor to 0.
 *   gdg_batch_dither_seek(ctx, sample_index)           the sample index the next gdg_batch_finish_master_slice starts at (a caller that
 *                                                      resumes a sharded job from a checkpoint seeks to samples_done).  The cursor is no
 *                                                      part of a streamed job: it may be set while one is open.
 * Configuration, like gdg_batch_report_enable and gdg_batch_set_sources: it holds from the next batch call on, survives batch calls and is
 * part of no blob (the checkpoint container stays version 1) -- set it again on the target of a resume.  The render report is taken from
 * the float64 rows, before the dither: its records are the same with dither on and off; so are the meters, and a NULL in out_bytes
 * changes nothing else.  Off -- never set, or mode 0 -- no launch, allocation, upload or byte differs from a context that never heard of
 * the call.  No noise shaping: error feedback is a serial recurrence per port that would carry state across slices.
 * The encoder on its own, mono, for callers with their own buffers:
 *   gdg_wave_encode_dither(ctx, format, samples, n, mode, seed, port, first_index, bytes)            host buffers, blocking
 *   gdg_wave_encode_dither_device(ctx, format, d_samples, n, mode, seed, port, first_index, d_bytes) enqueued on gdg_ctx_stream; any
 *                                                      8-byte alignment of d_samples, any byte alignment of d_bytes
 * sample i of the buffer has index first_index + i.  mode 0, or an IEEE format, gives gdg_wave_encode's bytes.
 */
int gdg_batch_set_dither(gdg_ctx *ctx, int mode, uint64_t seed, uint32_t port_base);
int gdg_batch_dither_seek(gdg_ctx *ctx, uint64_t sample_index);
int gdg_wave_encode_dither(gdg_ctx *ctx, int format, const double *samples, size_t n, int mode, uint64_t seed, uint32_t port, uint64_t first_index,
                           void *bytes);
int gdg_wave_encode_dither_device(gdg_ctx *ctx, int format, const double *d_samples, size_t n, int mode, uint64_t seed, uint32_t port,
                                  uint64_t first_index, void *d_bytes);
/*
 * TRIM: no reference counterpart.  The batch calls measure what they render -- peak, RMS and clip counts, bands, lag and polarity, true peak
 * -- and the trim acts on those numbers where it costs nothing and loses nothing: one gain per output port in front of the encoders, read
 * from the float64 rows as they lie on the device.  A file that would clip in the encoder's clamp is written below full scale instead, a
 * quiet rig keeps the bits a 16-bit truncation would drop, an inverted rig is written upright.  Stateless per sample: no place in the
 * checkpoint, no rule for windows, slices or shards, no change to the container version.
 *   gdg_batch_set_trim(ctx, chain_gain, n, master_left, master_right, metronome)
 *                                                      chain_gain: n gains, n = the context's channel count -- the gains of the
 *                                                      context's OWN chain outputs (a shard passes its own channels');
 *                                                      chain_gain == NULL with n == 0: every chain gain is 1.  The three scalars are
 *                                                      the gains of the job-wide ports.  Every gain is finite; a negative gain inverts
 *                                                      the polarity; zero is allowed.
 * GDG_ERR_INVALID, with gdg_last_error naming the offending entry, and the setting in force unchanged: a gain that is not finite, a wrong
 * n, a call while a streamed job is open.
 * OFF: all gains equal to 1.0, or never called.  Off, no launch, allocation, upload or byte differs from a context that never heard of
 * the call; option stat_batch_device_kib is unchanged and the existing kernels are dispatched unchanged.
 * Configuration, like gdg_batch_set_dither: it holds from the next batch call on, survives batch calls and is part of no blob -- set it
 * again on the target of a resume.
 * DEFINITION, for a sample x of a port with gain g:
 *   y = x * g                                          ONE IEEE-754 double multiply, rounded once; never contracted with what follows (no
 *                                                      fused multiply-add with the encoder's scale S)
 * and the encoder does with y exactly what it does with x without a trim: the plain encoders clamp, scale and truncate toward zero; the
 * dither encoders (DITHER, above) compute t = S * clamp1(y), q = floor((t + d) + 0.5) with the noise d of the same (seed, port, index);
 * IEEE32 and IEEE64 go through their conversion and clipping rule, applied to y (IEEE32: (float)clamp1(y); IEEE64: y's 8 bytes).  A gain
 * of exactly 1.0 gives the bytes of off for every finite sample.
 * WHERE:
 *   gdg_batch_run, gdg_batch_stream_step                           the N chain outputs, master left, master right, metronome
 *   gdg_batch_run_shard, gdg_batch_stream_step_shard               the n chain outputs and metronome_bytes
 *   gdg_batch_finish_master, gdg_batch_finish_master_slice         left_bytes and right_bytes, with the master_left / master_right gains
 *                                                                  of the context that finishes
 * WHAT NEVER CHANGES: the float64 rows, the master mix, a shard's float64 partial master and its float64 metronome, the meters, the tuner
 * rings, the channel state, and all four record kinds -- report, spectrum, alignment, true peak: they describe the render, BEFORE the trim.
 * Nothing changes for a NULL in out_bytes.
 * What lets a caller predict the written file: rounding is monotone, so the largest written magnitude of a block is exactly
 * fl(|g| * peak), clamped to 1 (peak: gdg_block_stats.peak); and with |g| * true_peak <= 1 no sample of the file is clipped.
 * Known answer: dither on, seed 0x63, port 3, index 8192, x = 2e-5, g = 0.5 gives DITHER's codes of x = 1e-5 -- LPCM16 code 0, LPCM24 code
 * 83 (a scaling by a power of two commutes with rounding).
 * The encoder on its own, mono, the sibling of gdg_wave_encode_dither(_device) with its alignment rules:
 *   gdg_wave_encode_trim(ctx, format, samples, n, gain, mode, seed, port, first_index, bytes)            host buffers, blocking
 *   gdg_wave_encode_trim_device(ctx, format, d_samples, n, gain, mode, seed, port, first_index, d_bytes) enqueued on gdg_ctx_stream
 * gain == 1.0 gives gdg_wave_encode_dither's bytes; mode 0 is the plain encoder applied to x * gain.  A gain that is not finite is
 * GDG_ERR_INVALID.
 * THE PLANNER, pure host arithmetic (csrc/trim.h), no context and no device:
 *   gdg_trim_from_true_peak(records, ports, blocks, target, max_gain, gain)
 *                                                      records: [ports][blocks] as gdg_batch_true_peak hands them out; gain: ports
 *                                                      doubles.  For each port m = the largest true_peak over its blocks; m == 0:
 *                                                      gain = 1.0; otherwise gain = min(target / m, max_gain).  blocks == 0: every
 *                                                      gain 1.0.  target and max_gain are finite and greater than 0; a NaN true_peak in
 *                                                      a record is refused: GDG_ERR_INVALID, nothing of `gain` written, and
 *                                                      gdg_last_error(NULL) of the calling thread names the port.
 * Known answers: maxima {0.5, 2.0, 0}, target 0.891250938, max_gain 4 give {1.782501876, 0.445625469, 1.0}; maxima {0.01}, the same
 * target and max_gain, give {4.0}.
 */
int gdg_batch_set_trim(gdg_ctx *ctx, const double *chain_gain, int n, double master_left, double master_right, double metronome);
int gdg_wave_encode_trim(gdg_ctx *ctx, int format, const double *samples, size_t n, double gain, int mode, uint64_t seed, uint32_t port,
                         uint64_t first_index, void *bytes);
int gdg_wave_encode_trim_device(gdg_ctx *ctx, int format, const double *d_samples, size_t n, double gain, int mode, uint64_t seed, uint32_t port,
                                uint64_t first_index, void *d_bytes);
int gdg_trim_from_true_peak(const gdg_block_true_peak *records, int ports, size_t blocks, double target, double max_gain, double *gain);
/*
 * BLEND: no reference counterpart.  A re-amping job renders one take through many rigs (gdg_batch_set_sources), and what its user does with
 * the renders is blend a few of them: two amps at 60/40, two microphone positions of one cabinet, a clean rig under a driven one.  A blend
 * output is a weighted sum of chain outputs, made from the float64 rows as they lie on the device -- before any of them is truncated to 16
 * or 24 bits -- and written as one more port behind the metronome's.  Stateless per sample while every delay is 0 (DELAYS, below): no place
 * in the checkpoint, no rule for windows or slices, the same bits however the job is cut, no change to the container version.
 *   gdg_batch_set_blends(ctx, n_blends, first, channel, weight, gain)
 *                                                      the blends in CSR form: blend b has the terms k = first[b] .. first[b + 1] - 1,
 *                                                      term k is channel[k] of THIS context with weight[k]; first has n_blends + 1
 *                                                      entries, starts at 0 and never descends.  gain: one output gain per blend, or
 *                                                      NULL: every gain 1.0.  n_blends == 0 turns the blends off (the lists may be NULL).
 *   gdg_batch_blends(ctx)                              the number of blends in force
 * LIMITS: 1 <= terms per blend <= GDG_BLEND_MAX_TERMS (32); 0 <= n_blends <= GDG_BLEND_MAX_BLENDS (1024); every channel lies in [0, N), N =
 * gdg_ctx_channels.  Weights and gains are finite; negative and zero values are allowed; a channel may appear more than once in a blend.
 * GDG_ERR_INVALID, with gdg_last_error naming the blend and the term, and the setting in force unchanged: a blend without a term or with
 * more than 32, a channel out of range, a weight or a gain that is not finite, a `first` that does not start at 0 or descends, a count
 * outside the limits, a call while a streamed job is open.  The whole argument is validated before it replaces the setting in force.
 * OFF: n_blends == 0, or never called.  Off, no launch, allocation, upload or byte differs from a context that never heard of the call, and
 * option stat_batch_device_kib is unchanged.
 * Configuration, like gdg_batch_set_trim and gdg_batch_set_sources: it holds from the next batch call on, survives batch calls and is part
 * of no blob -- set it again on the target of a resume.
 * DEFINITION, for every sample index i of the job, with x[c] the float64 chain output row of channel c -- the row the encoder reads: before
 * the trim, before the spatializer:
 *   s = w_0 * x[c_0][i]                                ONE rounded IEEE-754 double multiply
 *   s = s + (w_k * x[c_k][i])      k = 1 .. K - 1      one rounded multiply, one rounded add, in term order
 * never contracted into a fused multiply-add and never reassociated.  s is the blend port's float64 row.  The port is encoded from
 *   y = s * g_b                                        exactly as the trim encodes x * g (TRIM, above): the plain or the dithered encoder, in
 *                                                      any of the six formats; IEEE64 writes y's 8 bytes
 * and with g_b == 1.0 from s itself.  NaN and inf in a row follow IEEE arithmetic; 0 * inf is NaN.  WHERE a sample of s is a NaN is defined;
 * the sign and the payload of a NaN the arithmetic produces are not (IEEE 754 leaves them open: 0 * inf is the negative quiet NaN on x86
 * and the positive one on gfx950), so the 8 bytes IEEE64 writes for such a sample are those of some NaN.
 * Known answer: weights {0.1, 0.2, 0.3} on three rows of 1.0 give 0.6000000000000001; the same terms in reverse order give 0.6.
 * PORTS: with B blends in force gdg_batch_run, gdg_batch_stream_step and the job of gdg_batch_stream_resume take out_bytes of N + 3 + B
 * entries: blend b is port N + 3 + b, behind the metronome's.  A NULL entry skips the file as for any port.
 *   records     gdg_batch_report, gdg_batch_spectrum, gdg_batch_align and gdg_batch_true_peak hand out N + 3 + B ports; a blend port's
 *               records are taken from s, before the gain, as the others are taken before the trim
 *   dither      blend b is port port_base + N + 3 + b of the dither, with the sample index in the job as ever; that range stays below the
 *               job-wide ports (refused when the job is described)
 *   alignment   gdg_batch_align_enable's n_ports is N + 3 or N + 3 + B for the B in force when a job is described.  With N + 3 every blend
 *               port references itself; with N + 3 + B a blend may name any port as its reference, one of its own terms included.  Any
 *               other count is refused when the job is described, with both numbers in the message.
 * WHAT NEVER CHANGES: the chain, master and metronome files of a job with blends are byte for byte those of the job without; the master
 * mix, the meters (still 2 N + 3 ports), the tuner and the channel state never see a blend.  The trim's gains are those of ports 0 .. N + 2;
 * a blend port has its own g_b.
 * SHARDS: gdg_batch_run_shard, gdg_batch_stream_open_shard and gdg_batch_stream_resume_shard return GDG_ERR_UNSUPPORTED while blends are in force
 * on their context; gdg_batch_stream_step_shard then never finds a job of theirs open (and the setting cannot change while one is).  A shard's row layout is a different problem, and a blend whose terms live
 * on two devices is another one.
 * The sum on its own, over any rows (`channel` then names a row: 0 .. n_rows - 1; no gain), both blocking -- the table is host memory:
 *   gdg_blend_rows(ctx, rows, n_rows, samples, n_blends, first, channel, weight, out)        host rows; out[b]: `samples` doubles
 *   gdg_blend_rows_device(ctx, d_rows, row_stride, n_rows, samples, n_blends, first, channel, weight, d_out, out_stride)
 *                                                      device rows, 8-byte aligned: row r at d_rows + r * row_stride, blend b's sums at
 *                                                      d_out + b * out_stride (strides in samples, >= samples); d_out overlaps no row
 * DELAYS: the alignment records say how far apart two renders of one take lie (ALIGNMENT, above); a delay per term lines them up before
 * they are summed.  Term k of a blend has an integer delay d_k, 0 <= d_k <= GDG_BLEND_MAX_DELAY (4096: the alignment measures lags within
 * +-2048, so two terms of one blend lie at most 4096 samples apart).  With i the sample index in the job:
 *   x_k[i] = x[c_k][i - d_k]       for i >= d_k
 *   x_k[i] = +0.0                  for i <  d_k
 *   s = w_0 * x_0[i]
 *   s = s + (w_k * x_k[i])         in term order
 * every product and every add rounded on its own exactly as above (0 * +0.0 is still a product: a negative weight in front of the job gives
 * -0.0).  The port's length stays the job's length: the last d_k samples of a delayed term are never written to any port.  Records, dither
 * ports, output gains and the alignment list are those of blend ports without delays.
 * Known answer: two terms on one row x with d = {0, 1} and weights {1, -1} give the first difference of the row: s[0] = x[0] - (+0.0) =
 * x[0], s[i] = x[i] - x[i - 1].
 *   gdg_batch_set_blends_delayed(ctx, n_blends, first, channel, weight, delay, gain)
 *                                                      gdg_batch_set_blends with one delay per term; delay == NULL: every delay 0, and
 *                                                      gdg_batch_set_blends is this call with delay == NULL.  A delay outside the range
 *                                                      is GDG_ERR_INVALID, names blend and term, and leaves the list in force unchanged.
 *   gdg_batch_blend_max_delay(ctx)                     the largest delay in force; 0: the blends are stateless
 * With every delay 0 no buffer, launch, upload byte or output byte differs from gdg_batch_set_blends.  With a delay in force the context
 * keeps the last GDG_BLEND_MAX_DELAY samples of its N chain rows from step to step and from slice to slice: N * 4096 doubles, counted by
 * stat_batch_device_kib, zeroed when a job begins (gdg_batch_run, the first slice after gdg_batch_stream_open), freed when the delays go back
 * to zero or the blends go off.  The bytes do not depend on the window or on how the job is sliced.
 * That history is not in the version-1 checkpoint container: while a non-zero delay is in force gdg_batch_stream_checkpoint_size,
 * gdg_batch_stream_checkpoint, gdg_batch_stream_resume and the shard forms return GDG_ERR_UNSUPPORTED and write nothing.  With every delay
 * 0 a checkpoint is what it was.
 * The delayed sum on its own, both blocking, refusing what gdg_blend_rows refuses and a delay out of range:
 *   gdg_blend_rows_delayed(ctx, rows, n_rows, samples, n_blends, first, channel, weight, delay, history, out)
 *                                                      history: NULL (zeros in front of sample 0) or n_rows pointers to
 *                                                      GDG_BLEND_MAX_DELAY doubles each: history[r][GDG_BLEND_MAX_DELAY - 1] is sample -1
 *                                                      of row r.  Read, never written.
 *   gdg_blend_rows_delayed_device(ctx, d_rows, row_stride, n_rows, samples, n_blends, first, channel, weight, delay, d_history, hist_stride,
 *                                 d_out, out_stride)   d_history: NULL or device memory, 8-byte aligned, row r's run at d_history + r *
 *                                                      hist_stride (hist_stride >= GDG_BLEND_MAX_DELAY); d_out overlaps neither side
 * The delays from the alignment records -- host only: no context, no device, like gdg_trim_from_true_peak (gdg_last_error(NULL) says what
 * was refused):
 *   gdg_blend_delays_from_align(records, ports, blocks, ref, min_coeff, n_blends, first, channel, delay, sign)
 *                                                      records[ports][blocks] as gdg_batch_align hands them out, ref: the list they were
 *                                                      measured with; the blends in CSR form, `channel` naming a port; delay and sign:
 *                                                      one int per term
 * Per port: the blocks with ref_sq > 0, sq_at_lag > 0 and |corr| / sqrt(ref_sq * sq_at_lag) >= min_coeff (0 <= min_coeff <= 1) count; the
 * port's lag is the lower median of `lag` over those blocks, its sign the sign of the sum of `corr` over them.  A port with no such block
 * gets lag 0 and sign +1, and so does a port that is its own reference or is the reference of the others.  Per blend: every term's
 * channel is measured against one reference port, or is that port; otherwise the call returns GDG_ERR_INVALID, writes nothing and names the
 * blend.  delay_k = max_j lag_j - lag_k; sign_k is the port's sign: the caller multiplies the weights by it.
 * FILTERS: a short FIR per term.  With windowed-sinc taps it is a fractional delay -- at 44.1 or 48 kHz half a sample of offset between two
 * microphone positions is 90 degrees at 11-12 kHz, the comb filter the alignment was built to remove, an octave up --, with other taps a
 * per-term tilt or match EQ, taken from the float64 rows before anything is truncated.  Term k of a blend has, beside c_k, w_k and d_k, a
 * tap count T_k, 0 <= T_k <= GDG_BLEND_MAX_TAPS (64), and taps h_k[0 .. T_k - 1].  The taps are finite doubles; zero and negative taps are
 * allowed.  With i the sample index in the job, and x[c][j] = +0.0 for j < 0:
 *   T_k == 0:  x_k[i] = x[c_k][i - d_k]                                  exactly DELAYS
 *   T_k >= 1:  f = h_k[0] * x[c_k][i - d_k]                              one rounded multiply
 *              f = f + (h_k[t] * x[c_k][i - d_k - t])    t = 1 .. T_k - 1   one rounded multiply, one rounded add, ascending t
 *              x_k[i] = f
 *   s = w_0 * x_0[i];  s = s + (w_k * x_k[i])   in term order            unchanged
 * Nothing is ever contracted into a fused multiply-add and nothing is reassociated (csrc/blend.h: gdg_blend_mul, gdg_blend_add).
 * The limit per term is d_k + max(T_k, 1) - 1 <= GDG_BLEND_MAX_DELAY: the term's REACH.  The history of [N][4096] doubles is therefore
 * enough, and it is used exactly as DELAYS uses it: allocated only while some term's reach is above 0, zeroed by the first slice of a job,
 * saved behind the sum of each step, counted by stat_batch_device_kib.
 * Known answer: one term on row x with d = 0, T = 2, h = {1, -1} and w = 1 gives s[0] = x[0] and s[i] = x[i] - x[i - 1]: the bits of the
 * DELAYS known answer.
 * Where a NaN lands is defined: a NaN at x[c][j] reaches i = j + d .. j + d + T - 1; its sign and payload are not, as elsewhere.
 * Ports, records, dither ports, output gains, the alignment list, fits and Gram lists treat a filtered blend port like any other blend
 * port: they read s, before g_b.
 *   gdg_batch_set_blends_filtered(ctx, n_blends, first, channel, weight, delay, tap_first, tap, gain)
 *                                                      tap_first: one entry per term plus one, in CSR form over all terms of all blends;
 *                                                      it starts at 0 and never descends; term k has the taps tap[tap_first[k] ..
 *                                                      tap_first[k + 1] - 1].  tap_first == NULL: the call IS
 *                                                      gdg_batch_set_blends_delayed -- the same table byte for byte, the same kernels and
 *                                                      buffers, the same bytes uploaded and written.  So is a list whose every T_k is 0.
 *   gdg_batch_blend_max_reach(ctx)                     the largest d_k + max(T_k, 1) - 1 in force; 0: the blends are stateless
 * Validation follows the delayed call: the whole argument is checked before anything replaces the setting in force; GDG_ERR_INVALID, with
 * gdg_last_error naming the blend and the term, and the setting unchanged: a tap that is not finite, a count above 64, a reach above 4096,
 * a tap_first that does not start at 0 or descends, a call while a streamed job is open.  gdg_batch_blend_max_delay keeps its meaning: the
 * largest d_k.  The checkpoint calls, gdg_batch_stream_resume and their shard forms return GDG_ERR_UNSUPPORTED while
 * gdg_batch_blend_max_reach > 0; the four shard calls refuse blends as ever.
 * The filtered sum on its own, both blocking, refusing what gdg_blend_rows_delayed refuses and the taps refused above:
 *   gdg_blend_rows_filtered(ctx, rows, n_rows, samples, n_blends, first, channel, weight, delay, tap_first, tap, history, out)
 *   gdg_blend_rows_filtered_device(ctx, d_rows, row_stride, n_rows, samples, n_blends, first, channel, weight, delay, tap_first, tap,
 *                                  d_history, hist_stride, d_out, out_stride)
 * The taps of a fractional delay and the fraction from fit records -- host only: no context, no device (gdg_last_error(NULL) says what was
 * refused):
 *   gdg_blend_fraction_taps(n_taps, fraction, tap)     T = n_taps even, 2 <= T <= 64; 0 <= fraction < 1.  The taps delay by T/2 - 1 +
 *                                                      fraction samples: sinc(u) * (0.5 + 0.5 cos(2 pi u / T)) with u = t - (T/2 - 1) -
 *                                                      fraction, divided by their sum.  fraction == 0 returns the exact unit impulse at
 *                                                      T/2 - 1, with no call into libm.
 *   gdg_blend_fractions_from_fit(records, n_fits, blocks, steps, step)
 *                                                      records[n_fits][blocks] of gdg_batch_fit (FIT, below); steps = Q, 1 <= Q <= 4.
 *                                                      Fit f has 2Q - 1 terms, term k the candidate at offset (k - (Q - 1)) / Q samples.
 * The records of the blocks are added in block order.  The candidate with the largest tx[k] / sqrt(xx[k][k]) wins; only candidates with
 * xx[k][k] > 0 count; the earlier entry wins a tie.  step[f] is its k - (Q - 1).  A fit with tt <= 0 or without an admissible candidate
 * gives 0.  A fit with another term count, or a non-finite sum, is refused whole and nothing is written.
 */
#define GDG_BLEND_MAX_TERMS 32
#define GDG_BLEND_MAX_BLENDS 1024
#define GDG_BLEND_MAX_DELAY 4096
#define GDG_BLEND_MAX_TAPS 64
int gdg_batch_set_blends(gdg_ctx *ctx, int n_blends, const int *first, const int *channel, const double *weight, const double *gain);
int gdg_batch_blends(const gdg_ctx *ctx);
int gdg_blend_rows(gdg_ctx *ctx, const double *const *rows, int n_rows, size_t samples, int n_blends, const int *first, const int *channel,
                   const double *weight, double *const *out);
int gdg_blend_rows_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, int n_blends, const int *first,
                          const int *channel, const double *weight, double *d_out, size_t out_stride);
int gdg_batch_set_blends_delayed(gdg_ctx *ctx, int n_blends, const int *first, const int *channel, const double *weight, const int *delay,
                                 const double *gain);
int gdg_batch_blend_max_delay(const gdg_ctx *ctx);
int gdg_blend_rows_delayed(gdg_ctx *ctx, const double *const *rows, int n_rows, size_t samples, int n_blends, const int *first, const int *channel,
                           const double *weight, const int *delay, const double *const *history, double *const *out);
int gdg_blend_rows_delayed_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, int n_blends, const int *first,
                                  const int *channel, const double *weight, const int *delay, const double *d_history, size_t hist_stride,
                                  double *d_out, size_t out_stride);
int gdg_blend_delays_from_align(const gdg_block_align *records, int ports, size_t blocks, const int *ref, double min_coeff, int n_blends,
                                const int *first, const int *channel, int *delay, int *sign);
int gdg_batch_set_blends_filtered(gdg_ctx *ctx, int n_blends, const int *first, const int *channel, const double *weight, const int *delay,
                                  const int *tap_first, const double *tap, const double *gain);
int gdg_batch_blend_max_reach(const gdg_ctx *ctx);
int gdg_blend_rows_filtered(gdg_ctx *ctx, const double *const *rows, int n_rows, size_t samples, int n_blends, const int *first, const int *channel,
                            const double *weight, const int *delay, const int *tap_first, const double *tap, const double *const *history,
                            double *const *out);
int gdg_blend_rows_filtered_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, int n_blends, const int *first,
                                   const int *channel, const double *weight, const int *delay, const int *tap_first, const double *tap,
                                   const double *d_history, size_t hist_stride, double *d_out, size_t out_stride);
int gdg_blend_fraction_taps(int n_taps, double fraction, double *tap);
/*
 * FIT: no reference counterpart.  The one blend parameter the records above do not measure is the weight: "which mix of these few rigs
 * comes closest to THAT track?" is a linear least-squares problem, and everything it needs is an inner product of float64 rows that already
 * lie in the batch window on the device, before anything is truncated to 16 or 24 bits.  A fit record holds those inner products per block;
 * a host planner turns the records into blend weights.  Stateless: a function of the block's samples alone -- a term that has to be delayed
 * or inverted first is fitted as the port of a one-term delayed blend (DELAYS, above).
 * INPUTS: a fit f has a target port t and terms p_0 .. p_{K-1}, 1 <= K <= GDG_FIT_MAX_TERMS (8).  Ports are rows of the batch window, 0 ..
 * N + 2 + B: chain outputs, master left, master right, metronome and the B blend ports.  A port may repeat; the target may be a term.  Up to
 * GDG_FIT_MAX_FITS (256) fits.  Rows are read as the record kernels read them: before the trim, and a blend port's s before g_b.
 * RECORD: per fit and block of 8192 samples one gdg_block_fit (below): tt = sum t[i]^2, tx[k] = sum t[i] * x_k[i], and the lower triangle
 * of the Gram matrix by rows, xx[j (j + 1) / 2 + k] = sum x_j[i] * x_k[i] for k <= j.  Entries for terms >= K are +0.0.  A sample index i
 * at which ANY of the fit's K + 1 rows is NaN or +-inf is left out of ALL 45 sums and counted in `skipped`.
 * ORDER OF THE SUMS: the block statistics' order, for every entry: one workgroup of 256 threads per (block, fit); thread t walks the sample
 * pairs t, t + 256, ... -- sample 2 p, then 2 p + 1 -- with one running sum per entry; the 64 lanes meet in the fixed tree lane i <- lane i +
 * 32, 16, ... 1; the four wave results are added in the order 0, 1, 2, 3.  Every product and every add is rounded on its own, never
 * contracted, and there are no floating-point atomics: nothing depends on the grid, the row, the window, the slice or arrival order.
 *   With skipped == 0, xx[k (k + 1) / 2 + k] is bit for bit the sum_sq of gdg_block_stats for port p_k and that block, and tt that of port t.
 *   xx is bitwise symmetric under exchanging two terms.
 *   The records are the same bits whatever the window, the slicing, a resume or a source map.
 *   gdg_batch_fit_enable(ctx, n_fits, first, port, target)
 *                                                      the fits in CSR form: fit f has the terms port[first[f]] .. port[first[f + 1] - 1]
 *                                                      and the target target[f]; first has n_fits + 1 entries, starts at 0 and never
 *                                                      descends.  n_fits == 0: off (the lists may be NULL).  Refused whole, with the fit
 *                                                      named and the list in force unchanged: a fit without a term or with more than 8, a
 *                                                      negative port, a broken `first`, a count outside 0 .. 256, a streamed job open.
 *   gdg_batch_fits(ctx)                                the number of fits in force
 *   gdg_batch_fit(ctx, records, capacity, &fits, &blocks)
 *                                                      the [fits][blocks] records of the LAST COMPLETED batch call; records == NULL: the
 *                                                      counts only.  GDG_ERR_INVALID when capacity < fits * blocks, or when there are no
 *                                                      records: no call has completed since the switch, or the last one was a master finish.
 * Port numbers are checked when a job is described -- gdg_batch_run, gdg_batch_stream_open, gdg_batch_stream_resume -- against N + 3 + B of
 * that call; a port at or beyond it is GDG_ERR_INVALID with the fit named.
 * OFF: n_fits == 0, or never called.  Off, no launch, buffer, upload byte or output byte differs from a context that never heard of the call,
 * and option stat_batch_device_kib is unchanged; on, it counts the fits' table and the records' room in the download halves.
 * Configuration, like the blends: it holds from the next batch call on, is part of no blob -- set it again on the target of a resume -- and a
 * checkpoint and a resume work with fits on.  The records come down with each step's own download, behind the four record kinds' sections.
 * SHARDS: gdg_batch_run_shard, gdg_batch_stream_open_shard, gdg_batch_stream_step_shard and gdg_batch_stream_resume_shard return
 * GDG_ERR_UNSUPPORTED while fits are in force on their context.  gdg_batch_finish_master and gdg_batch_finish_master_slice never collect fits.
 * The record on its own, over any rows and any block length >= 1 (ports name rows 0 .. n_rows - 1; the last block of a row may be short);
 * both blocking -- the table is host memory:
 *   gdg_block_fit_rows(ctx, rows, n_rows, samples, block, n_fits, first, port, target, records)
 *                                                      host rows of `samples` float64; records: [n_fits][ceil(samples / block)]
 *   gdg_block_fit_rows_device(ctx, d_rows, row_stride, n_rows, samples, block, n_fits, first, port, target, d_records)
 *                                                      device rows, 8-byte aligned: row r at d_rows + r * row_stride (row_stride >=
 *                                                      samples); no sample outside [row, row + samples) is read; d_records: device
 *                                                      memory, 8-byte aligned
 * THE PLANNER, pure host arithmetic (csrc/blend.h), no context and no device (gdg_last_error(NULL) says what was refused):
 *   gdg_blend_weights_from_fit(records, n_fits, blocks, ridge, weight, residual)
 *                                                      records[n_fits][blocks] as gdg_batch_fit hands them out, blocks >= 1;
 *                                                      weight[n_fits][8], residual[n_fits]
 * Per fit: the blocks' records are added in block order with plain double adds: T, b[K], G[K][K].  (G + ridge * mean(diag G) * I) w = b is
 * solved by an unpivoted Cholesky factorisation in term order; ridge >= 0 and finite.  A pivot <= K * 2^-52 * max(diag G) -- a silent term,
 * or a port used twice with ridge = 0 -- is GDG_ERR_INVALID: nothing is written and the fit is named.  residual = max(0, T - 2 w.b + w'Gw)
 * / T, and 0 when T == 0: the share of the target's energy that the fitted blend leaves.  Weights of terms >= K are 0.
 * Known answers: one term with G = 4 and b = 2 gives w = 0.5; two orthogonal terms with G = diag(4, 1), b = {2, 3} and T = 10 give w =
 * {0.5, 3} and residual 0; a target that is term 0 gives w = {1, 0, ..} and residual 0; one port twice with G = 4 everywhere, b = {2, 2}
 * is refused with ridge = 0 and gives two equal weights with ridge > 0.
 */
#define GDG_FIT_MAX_TERMS 8
#define GDG_FIT_MAX_FITS 256
typedef struct gdg_block_fit {
    double   tt;          /* sum t[i]^2 */
    double   tx[8];       /* tx[k] = sum t[i] * x_k[i] */
    double   xx[36];      /* lower triangle by rows: xx[j (j + 1) / 2 + k] = sum x_j[i] * x_k[i], k <= j */
    uint32_t skipped;     /* sample indices left out of every sum: some row of the fit was NaN or +-inf there */
    uint32_t terms;       /* K */
} gdg_block_fit;          /* 368 bytes, little-endian, no padding */
int gdg_batch_fit_enable(gdg_ctx *ctx, int n_fits, const int *first, const int *port, const int *target);
int gdg_batch_fits(const gdg_ctx *ctx);
int gdg_batch_fit(gdg_ctx *ctx, gdg_block_fit *records, size_t capacity, int *fits, size_t *blocks);
int gdg_block_fit_rows(gdg_ctx *ctx, const double *const *rows, int n_rows, size_t samples, int block, int n_fits, const int *first, const int *port,
                       const int *target, gdg_block_fit *records);
int gdg_block_fit_rows_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, int block, int n_fits, const int *first,
                              const int *port, const int *target, gdg_block_fit *d_records);
int gdg_blend_weights_from_fit(const gdg_block_fit *records, int n_fits, size_t blocks, double ridge, double *weight, double *residual);
/* BLEND, FILTERS: the fraction of a delay from the records of one fit per channel */
int gdg_blend_fractions_from_fit(const gdg_block_fit *records, int n_fits, size_t blocks, int steps, int *step);
/*
 * GRAM: no reference counterpart.  A fit needs its 1 to 8 term ports named.  The question in front of it -- "which few of these many rigs, in
 * which mix, come closest to THAT track?" -- needs one object: the Gram matrix G = X X' of all candidate rows and the target.  A Gram record
 * holds it per block for one list of ports; a host planner picks up to 8 of them greedily from the records and returns their weights.
 * Stateless: a function of the block's samples alone.  A delayed or inverted candidate is listed as the port of a one-term delayed blend.
 * LIST: gdg_batch_gram_enable names ONE list of 2 to GDG_GRAM_MAX_PORTS (512) ports.  Ports are rows of the batch window, 0 .. N + 2 + B: chain
 * outputs, master left, master right, metronome and the B blend ports, read as the record kernels read them: before the trim, a blend port's
 * s before g_b.  A port that repeats an earlier entry is refused.
 * RECORD: per block of 8192 samples the lower triangle of the P x P Gram matrix of the listed rows over that block: P (P + 1) / 2 doubles,
 * entry (i, j), j <= i, at index i (i + 1) / 2 + j -- the fit's xx layout --, i and j positions in the list.  No header and no counts.  A NaN
 * or inf sample makes the entries of its row whatever IEEE arithmetic makes them: the block statistics count non-finite samples per port,
 * and the planner refuses a Gram it cannot use.
 * ORDER OF THE SUM: the sums are made by the FP64 matrix instruction v_mfma_f64_16x16x4_f64.  Entry (i, j) of a block is one accumulator
 * chain of that instruction, started at +0.0, over k = 0, 4, 8, ... ascending: each step adds the four products x_i[k + m] * x_j[k + m], m = 0
 * .. 3, to the accumulator as the instruction does (fused, not rounded one by one).  Samples behind the block's end count as +0.0.  The sum
 * is never split over k across waves or workgroups, uses no atomics and is never finished by a second pass: an entry depends on the block's
 * samples of its two rows and on nothing else -- not on P, the positions in the list, the window, the slicing, a resume, a source map or the grid.
 *   The entry is NOT bit for bit the sum_sq of gdg_block_stats, nor the xx of a gdg_block_fit: the order differs and the products are fused.
 *   It is within L * 2^-52 * sum_k |x_i[k] x_j[k]| of the exact sum for a block of L samples.
 *   The records are the same bits whatever the window, the slicing, a resume or a source map, and those of gdg_block_gram_rows on the same rows.
 *   gdg_batch_gram_enable(ctx, port, n_ports)          the list; n_ports == 0: off (port may be NULL).  Refused whole, with the entry named and
 *                                                      the list in force unchanged: a count of 1 or above 512, a negative port, a repeat, a
 *                                                      streamed job open.
 *   gdg_batch_gram_ports(ctx, port, capacity)          returns the number of ports in force and writes the first `capacity` of them (port may be NULL)
 *   gdg_batch_gram(ctx, out, capacity, &blocks)        the [blocks][P (P + 1) / 2] doubles of the LAST COMPLETED batch call, P the list in force --
 *                                                      setting a list drops the records of the one before; out == NULL: the count only;
 *                                                      capacity in doubles.  GDG_ERR_INVALID when capacity is too small, or when there are no
 *                                                      records: no call has completed since the switch, or the last one was a master finish.
 * Port numbers are checked when a job is described -- gdg_batch_run, gdg_batch_stream_open, gdg_batch_stream_resume -- against N + 3 + B of
 * that call; a port at or beyond it is GDG_ERR_INVALID with the entry named.
 * OFF: n_ports == 0, or never called.  Off, no launch, buffer, upload byte or output byte differs from a context that never heard of the call,
 * and option stat_batch_device_kib is unchanged; on, it counts the list and the records' room in the download halves.
 * SIZE: at P = 512 a record is 1 050 624 bytes.  Each of the two download halves grows by window x that (16.8 MB at a window of 16), every
 * step brings its records down with its rows, and the host keeps the whole call's records until the next batch call: 1 MiB per block, 128
 * MiB for a call of 128 blocks (22 s at 48 kHz).  A long job should run streamed and add each slice's records into one sum on the host.
 * Configuration, like the fits: it holds from the next batch call on, is part of no blob -- set it again on the target of a resume -- and a
 * checkpoint and a resume work with a list on.  The records come down with each step's own download, behind the fit section.
 * SHARDS: gdg_batch_run_shard, gdg_batch_stream_open_shard, gdg_batch_stream_step_shard and gdg_batch_stream_resume_shard return
 * GDG_ERR_UNSUPPORTED while a Gram list is in force on their context.  gdg_batch_finish_master and gdg_batch_finish_master_slice never collect Gram records.
 * The record on its own, over any rows and any block length >= 1 (a list of 1 to 512 entries naming rows 0 .. n_rows - 1; the last block of
 * a row may be short); both blocking -- the list is host memory:
 *   gdg_block_gram_rows(ctx, rows, n_rows, samples, block, port, n_ports, records)
 *                                                      host rows of `samples` float64; records: [ceil(samples / block)][P (P + 1) / 2]
 *   gdg_block_gram_rows_device(ctx, d_rows, row_stride, n_rows, samples, block, port, n_ports, d_records)
 *                                                      device rows, 8-byte aligned: row r at d_rows + r * row_stride (row_stride >=
 *                                                      samples); no sample outside [row, row + samples) is read; d_records: device
 *                                                      memory, 8-byte aligned
 * THE PLANNER, pure host arithmetic (csrc/blend.h), no context and no device (gdg_last_error(NULL) says what was refused):
 *   gdg_blend_pick_from_gram(records, n_ports, blocks, target, candidate, n_candidates, max_terms, ridge, min_gain, picked, weight, residual, &n_picked)
 *                                                      records[blocks][P (P + 1) / 2] as gdg_batch_gram hands them out, blocks >= 1; target
 *                                                      and candidate[n_candidates] are positions in the list; picked[8], weight[8], residual[8]
 * The blocks' records are added in block order with plain double adds.  T = G[target][target]; T <= 0 is refused, and so is a NaN or inf among
 * the entries of the target and the candidates, with the list position named, a candidate that is the target or repeats an earlier one, and
 * max_terms outside 1 .. 8.  Nothing is written on a refusal.  Greedy forward selection: with the set S picked so far, in pick order, every
 * candidate not in S is tried in list order: the unpivoted Cholesky factor of G_S + ridge * mean(diag) * I is extended by the candidate's row
 * -- the fit planner's solve on S and the candidate.  A candidate that brings a pivot at or below the fit planner's bound, K * 2^-52 * max(diag)
 * for the K rows then in the factor, is skipped, not refused: a silent rig, or a duplicate of a picked one.  r_c = max(0, T - 2 w.b + w'Gw) /
 * T; the smallest r_c wins, ties go to the earlier list entry.  It stops after max_terms picks, when the best candidate improves the
 * residual by less than min_gain (the residual before the first pick is 1), or when no candidate is admissible.  picked[m] is the list
 * position of pick m, residual[m] the share left after it; entries behind n_picked are -1, 0.0 and 0.0.  The weights are, bit for bit, what
 * gdg_blend_weights_from_fit returns for a gdg_block_fit holding the same sums of the picked ports in pick order.
 */
#define GDG_GRAM_MAX_PORTS 512
int gdg_batch_gram_enable(gdg_ctx *ctx, const int *port, int n_ports);
int gdg_batch_gram_ports(const gdg_ctx *ctx, int *port, int capacity);
int gdg_batch_gram(gdg_ctx *ctx, double *out, size_t capacity, size_t *blocks);
int gdg_block_gram_rows(gdg_ctx *ctx, const double *const *rows, int n_rows, size_t samples, int block, const int *port, int n_ports, double *records);
int gdg_block_gram_rows_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, int block, const int *port, int n_ports,
                               double *d_records);
int gdg_blend_pick_from_gram(const double *records, int n_ports, size_t blocks, int target, const int *candidate, int n_candidates, int max_terms, double ridge,
                             double min_gain, int *picked, double *weight, double *residual, int *n_picked);
/*
 * TAPFIT: no reference counterpart.  gdg_batch_set_blends_filtered gives every blend term up to 64 taps; until here the only taps the library
 * could make were windowed sincs.  "Which T-tap filter on this rig, or on these two microphone positions, comes closest to THAT track?" is
 * the fit's and the pick's normal-equations problem over shifted copies of a row.  A tap-fit record holds its sums per block; a host planner
 * solves them for the taps.  Stateless: a function of the block's samples alone.
 * FIT: a tap fit f has a target port t, term ports p_0 .. p_(K-1) and a tap count T, the same for all its terms: 1 <= K <=
 * GDG_TAPFIT_MAX_TERMS (4), 1 <= T <= GDG_BLEND_MAX_TAPS (64), U = K T <= GDG_TAPFIT_MAX_UNKNOWNS (128); up to GDG_TAPFIT_MAX_FITS (16) fits.
 * Ports are rows of the batch window, 0 .. N + 2 + B, read as the record kernels read them: before the trim, a blend port's s before g_b.  A
 * port may repeat and the target may be a term: the planner refuses what it cannot solve.
 * VIRTUAL ROWS: V = U + 1.  Row v = j T + a is term j at lag a, a = 0 .. T - 1; row U is the target at lag 0.  For a block of L samples that
 * starts at `first`, n = 0 .. L - T and i = first + T - 1 + n: row (j, a) has the value x[p_j][i - a], the target x[t][i].  Nothing outside
 * [first, first + L) is ever read: the first T - 1 samples of a block appear only as lags (stateless, like the 23 intervals the true peak
 * skips).  L < T: every entry is +0.0.
 * RECORD: the lower triangle of the V x V Gram matrix of the virtual rows, V (V + 1) / 2 doubles, entry (u, v), v <= u, at u (u + 1) / 2 + v --
 * the Gram record's layout.  No header.  A block's record is the concatenation over the fits in list order: D = sum_f V_f (V_f + 1) / 2
 * doubles per block (gdg_tapfit_doubles).
 * ORDER OF THE SUM: the Gram record's.  Entry (u, v) is one accumulator chain of v_mfma_f64_16x16x4_f64 started at +0.0 over n = 0, 4, 8, ...
 * ascending; positions behind L - T count as +0.0.  The chain is never split over waves or workgroups, uses no atomics and has no second
 * pass: an entry depends on the block's samples of its two ports, the two lags and T, and on nothing else -- not on K, the fit's position,
 * the other fits, the window, the slicing, a resume, a source map or the grid.  Two consequences:
 *   With T = 1 and different ports the record is bit for bit the gdg_block_gram_rows record of the list { p_0 .. p_(K-1), t }.
 *   For any T the record of one block is bit for bit what gdg_block_gram_rows returns for the V shifted rows written out on the host
 *   (row_v[n] as above, L - T + 1 samples, block = L - T + 1).
 * The fits come in CSR form, like the blend fits: fit f has the terms port[first[f] .. first[f + 1]), the target target[f] and taps[f] = T.
 *   gdg_batch_tapfit_enable(ctx, n_fits, first, port, target, taps)
 *                                                      the list; n_fits == 0: off (the lists may be NULL).  The whole list is validated
 *                                                      before it replaces the list in force; GDG_ERR_INVALID names the fit and the term.
 *                                                      Refused while a streamed job is open.
 *   gdg_batch_tapfits(ctx)                             the number of tap fits in force
 *   gdg_batch_tapfit(ctx, out, capacity, &blocks, &doubles_per_block)
 *                                                      the [blocks][D] doubles of the LAST COMPLETED batch call; out == NULL: the counts
 *                                                      only; capacity in doubles.  GDG_ERR_INVALID when capacity is too small, or when there
 *                                                      are no records: no call has completed since the switch, or the last one was a master finish.
 *   gdg_tapfit_doubles(n_fits, first, taps)            D, pure arithmetic (0 for no fit)
 * Port numbers are checked when a job is described -- gdg_batch_run, gdg_batch_stream_open, gdg_batch_stream_resume -- against N + 3 + B of
 * that call; a port at or beyond it is GDG_ERR_INVALID with the fit and the term named.
 * OFF: n_fits == 0, or never called.  Off, no launch, buffer, upload byte or output byte differs from a context that never heard of the call,
 * and option stat_batch_device_kib is unchanged; on, it counts the table and the records' room in the download halves.
 * Configuration, like the fits: it holds from the next batch call on, is part of no blob -- set it again on the target of a resume -- and a
 * checkpoint and a resume work with tap fits on.  The records come down with each step's own download, behind the Gram section.
 * SHARDS: gdg_batch_run_shard, gdg_batch_stream_open_shard, gdg_batch_stream_step_shard and gdg_batch_stream_resume_shard return
 * GDG_ERR_UNSUPPORTED while tap fits are in force on their context.  gdg_batch_finish_master and gdg_batch_finish_master_slice never collect tap-fit records.
 * The record on its own, over any rows and any block length >= 1 (ports name rows 0 .. n_rows - 1; the last block of a row may be short);
 * both blocking -- the lists are host memory:
 *   gdg_block_tapfit_rows(ctx, rows, n_rows, samples, block, n_fits, first, port, target, taps, records)
 *                                                      host rows of `samples` float64; records: [ceil(samples / block)][D]
 *   gdg_block_tapfit_rows_device(ctx, d_rows, row_stride, n_rows, samples, block, n_fits, first, port, target, taps, d_records)
 *                                                      device rows, 8-byte aligned: row r at d_rows + r * row_stride (row_stride >=
 *                                                      samples); no sample outside [row, row + samples) is read; d_records: device
 *                                                      memory, 8-byte aligned
 * THE PLANNER, pure host arithmetic (csrc/blend.h), no context and no device (gdg_last_error(NULL) says what was refused):
 *   gdg_blend_taps_from_tapfit(records, n_fits, first, taps, blocks, ridge, tap, residual)
 *                                                      records[blocks][D] as gdg_batch_tapfit hands them out, blocks >= 1; tap gets U_f
 *                                                      doubles per fit, concatenated, term by term, lag ascending; residual[n_fits]
 * Per fit the blocks' records are added in block order with plain double adds.  A = G[0 .. U)[0 .. U), b = G[U][0 .. U), Tt = G[U][U];
 * (A + ridge * mean(diag A) * I) h = b is solved by an unpivoted Cholesky factorisation in virtual-row order.  A pivot at or below U * 2^-52 *
 * max(diag A) is refused -- nothing is written, and the fit, the term and the lag are named -- and so is a NaN or inf entry.  residual =
 * max(0, Tt - 2 h.b + h'Ah) / Tt, and 0 when Tt == 0.  This is the fit planner's solve at any size: for U <= 8 the taps are bit for bit the
 * weights gdg_blend_weights_from_fit returns for a gdg_block_fit holding the same sums.  The taps are used as they come: term j of the blend
 * is (p_j's channel, weight 1.0, delay d_j, h_j) of gdg_batch_set_blends_filtered.
 * CONDITIONING: band-limited material -- a low-passed rig, an oversampled track -- makes the shifted copies of a row nearly dependent and A
 * ill-conditioned: the taps then carry large, cancelling values, or a pivot is refused.  ridge > 0 is the remedy; 1e-9 .. 1e-6 is a usual range.
 */
#define GDG_TAPFIT_MAX_TERMS 4
#define GDG_TAPFIT_MAX_UNKNOWNS 128
#define GDG_TAPFIT_MAX_FITS 16
int gdg_batch_tapfit_enable(gdg_ctx *ctx, int n_fits, const int *first, const int *port, const int *target, const int *taps);
int gdg_batch_tapfits(const gdg_ctx *ctx);
int gdg_batch_tapfit(gdg_ctx *ctx, double *out, size_t capacity, size_t *blocks, size_t *doubles_per_block);
int gdg_block_tapfit_rows(gdg_ctx *ctx, const double *const *rows, int n_rows, size_t samples, int block, int n_fits, const int *first, const int *port,
                          const int *target, const int *taps, double *records);
int gdg_block_tapfit_rows_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, int block, int n_fits, const int *first,
                                 const int *port, const int *target, const int *taps, double *d_records);
size_t gdg_tapfit_doubles(int n_fits, const int *first, const int *taps);
int gdg_blend_taps_from_tapfit(const double *records, int n_fits, const int *first, const int *taps, size_t blocks, double ridge, double *tap, double *residual);
/*
 * TRANSFER: no reference counterpart.  "Make this rig sound like that track" is a match EQ: a transfer function estimated over the whole
 * band and turned into an impulse response of hundreds to thousands of taps.  The tap fit stops at 128 unknowns and the band spectrum keeps
 * no phase.  A transfer record is the frequency-domain twin of the fit record: per block the two auto-spectra and the complex cross-spectrum
 * of a port against a target; summed over blocks they give the H1 estimate Sxy / Sxx and a coherence, and a host planner turns them into a
 * FIR that gdg_unit_set_fir takes like any other impulse response.  Stateless: a function of the block's samples alone.
 * LIST: 1 <= n_pairs <= GDG_TRANSFER_MAX_PAIRS (16) pairs (port[i], target[i]) and ONE group width D for the list, D in {1, 2, 4, 8, 16, 32,
 * 64}.  port == target is allowed, and a port may repeat.  Ports are rows of the batch window, 0 .. N + 2 + B, read as the record kernels read
 * them: before the trim, a blend port's s before g_b.
 * RECORD: the block length is L = 8192 (GDG_TRANSFER_BLOCK) always.  For block b, x is the block of row `port` and y the block of row
 * `target`; NaN and +-inf are taken as 0; a short last block is zero-padded.  Then
 *   w[n] = 0.5 - 0.5 cos(2 pi n / L)                        the periodic Hann window, the band spectrum's
 *   X[k] = sum_n w[n] x[n] exp(-2 pi i k n / L), Y[k] likewise, k = 0 .. L/2
 *   S = L^2 * 3/8;  Pxx[k] = |X[k]|^2 / S;  Pyy[k] = |Y[k]|^2 / S;  Pxy[k] = conj(X[k]) Y[k] / S
 * There is no doubling of the inner bins: these are sums to be divided, not powers to be read.  Im Pxy[0] = Im Pxy[L/2] = +0.0.
 * GROUPS: Gm = 4096 / D, groups g = 0 .. Gm, G = Gm + 1.  Group g is the sum over the bins g D - (D - 1) / 2 .. g D + D / 2 (integer division),
 * clipped to 0 .. 4096; D = 1 gives one bin per group; every bin lies in exactly one group.  The record of a pair and block is [G][4] doubles,
 * Sxx[g], Syy[g], Re Sxy[g], Im Sxy[g]; the record of the list and block is the pairs' parts concatenated in list order: n_pairs * G * 4
 * doubles (gdg_transfer_doubles), 131 104 bytes per pair at D = 1.  No header.
 * ORDER OF THE SUM: a group's four sums start at +0.0 and are added over ascending k; every product and every add is rounded on its own (no
 * contraction), no atomics.  An entry is a function of the two blocks' samples and D alone -- not of the pair's place in the list, the other
 * pairs, the row, the grid, the batch window, the slicing, a resume or the source map.
 * A SILENT SIDE: if all windowed samples of a side are zero after the non-finite rule, every entry that involves it is exactly +0.0; no
 * transform rounding from the other side leaks in.
 * UNEQUAL LEVELS: the two sides share one complex transform; each side is brought below 2 by an exact power of two of its own (from its
 * largest windowed magnitude) before the transform and the sums are scaled back by the same powers, so a port 2^-30 times the size of its
 * target keeps its Sxx to the transform's relative accuracy, measured against its OWN total.  SUPPORTED RANGE: the division by S acts
 * on the SCALED values (of a size near 1), and the powers go back on afterwards, one factor at a time -- exactly, as long as the entry itself
 * is a normal double.  That holds for a side whose largest windowed magnitude lies in 2^-480 .. 2^480; beyond it the entries -- squares of
 * the samples -- leave the doubles' range themselves: they lose bits or become 0 below, inf above.
 * KNOWN ANSWERS: x a cosine of amplitude 0.5 at bin 100 (x[n] = 0.5 cos(2 pi 100 n / L)) and y the sine there: at D = 1, Sxx = 0.25/24, 0.25/6,
 * 0.25/24 in groups 99, 100, 101, Re Sxy[100] = 0 and Im Sxy[100] = -0.25/6.  At D = 4 the three bins lie in group 25 (bins 99 .. 102): Sxx[25] =
 * 0.25/4 + 0 (bin 102 is empty).  PARSEVAL, in the raw form: sum_g Sxx[g] = ( L sum_n (w[n] x[n])^2 + |X[0]|^2 + |X[L/2]|^2 ) / (2 S) -- that is,
 * sum (w x)^2 / (L * 3/8) minus half of what bins 1 .. 4095 would carry doubled.
 *   gdg_batch_transfer_enable(ctx, n_pairs, port, target, group)
 *                                                      the list; n_pairs == 0 or port == NULL: off.  The whole list is validated before it
 *                                                      replaces the list in force; GDG_ERR_INVALID names the pair.  Refused while a streamed
 *                                                      job is open.
 *   gdg_batch_transfers(ctx)                           the number of pairs in force
 *   gdg_batch_transfer(ctx, out, capacity, &blocks, &doubles_per_block)
 *                                                      the [blocks][n_pairs][G][4] doubles of the LAST COMPLETED batch call; out == NULL: the
 *                                                      counts only; capacity in doubles.  GDG_ERR_INVALID when capacity is too small, or when
 *                                                      there are no records: no call has completed since the switch, or the last one was a master finish.
 *   gdg_transfer_doubles(n_pairs, group)               n_pairs (4096 / D + 1) 4, pure arithmetic (0 for no pair or a width that is none)
 * Port numbers are checked when a job is described -- gdg_batch_run, gdg_batch_stream_open, gdg_batch_stream_resume -- against N + 3 + B of
 * that call; a port at or beyond it is GDG_ERR_INVALID with the pair named.  Blend ports may be named.
 * OFF: no launch, buffer, upload byte or output byte differs from a context that never heard of the call, and option stat_batch_device_kib is
 * unchanged; on, it counts the table and the records' room in the download halves.
 * Configuration, like the fits: it holds from the next batch call on, is part of no blob -- set it again on the target of a resume -- and a
 * checkpoint and a resume work with a list in force.  The records come down with each step's own download, behind the tap-fit section.
 * SHARDS: gdg_batch_run_shard, gdg_batch_stream_open_shard, gdg_batch_stream_step_shard and gdg_batch_stream_resume_shard return
 * GDG_ERR_UNSUPPORTED while a transfer list is in force on their context.  gdg_batch_finish_master and gdg_batch_finish_master_slice never collect transfer records.
 * The record on its own, over any rows (ports name rows 0 .. n_rows - 1; the last block of a row may be short); both blocking -- the lists are
 * host memory, and the whole list is checked before anything is launched:
 *   gdg_block_transfer_rows(ctx, rows, n_rows, samples, n_pairs, port, target, group, records)
 *                                                      host rows of `samples` float64; records: [ceil(samples / 8192)][n_pairs][G][4]
 *   gdg_block_transfer_rows_device(ctx, d_rows, row_stride, n_rows, samples, n_pairs, port, target, group, d_records)
 *                                                      device rows, 8-byte aligned: row r at d_rows + r * row_stride (row_stride >=
 *                                                      samples); no sample outside [row, row + samples) is read; d_records: device
 *                                                      memory, 8-byte aligned
 * THE PLANNER, pure host arithmetic (csrc/blend.h), no context and no device (gdg_last_error(NULL) says what was refused):
 *   gdg_match_taps_from_transfer(records, n_pairs, group, blocks, ridge, n_taps, center, tap, coherence)
 *                                                      records[blocks][n_pairs][G][4] as gdg_batch_transfer hands them out, blocks >= 1;
 *                                                      tap[n_pairs][n_taps], coherence[n_pairs]
 * Per pair the blocks' records are added in block order with plain double adds.  N' = 2 Gm.  H[g] = Sxy[g] / (Sxx[g] + ridge * mean_g Sxx), 0
 * where the denominator is 0; the imaginary parts at g = 0 and g = Gm are dropped.  h is the inverse real transform of length N' (a host
 * float64 radix-2 decimation-in-time transform of the Hermitian extension).  tap[m] = t[m] * h[(m - center) mod N'] for m = 0 .. n_taps - 1, 1 <=
 * n_taps <= N' / 2, 0 <= center < n_taps, with the taper t[m] = 0.5 + 0.5 cos(pi (m - center) / E), E = center + 1 in front of the centre and
 * E = n_taps - center behind it: 1 at the centre and never 0 inside.  coherence = sum_g (|Sxy[g]|^2 / Sxx[g]) / sum_g Syy[g] over the groups with
 * Sxx[g] > 0: the share of the target's energy a linear filter on the port explains.  The coherence is 1 by construction for one block at
 * D = 1 (|Sxy|^2 = Sxx Syy bin by bin); averaging over blocks or groups is what makes it a measurement.  A NaN or inf entry is refused with
 * the pair named, and so is a pair with no energy in the port; nothing is written on a refusal.
 */
#define GDG_TRANSFER_BLOCK 8192
#define GDG_TRANSFER_MAX_PAIRS 16
#define GDG_TRANSFER_MAX_GROUP 64
int gdg_batch_transfer_enable(gdg_ctx *ctx, int n_pairs, const int *port, const int *target, int group);
int gdg_batch_transfers(const gdg_ctx *ctx);
int gdg_batch_transfer(gdg_ctx *ctx, double *out, size_t capacity, size_t *blocks, size_t *doubles_per_block);
int gdg_block_transfer_rows(gdg_ctx *ctx, const double *const *rows, int n_rows, size_t samples, int n_pairs, const int *port, const int *target, int group,
                            double *records);
int gdg_block_transfer_rows_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, int n_pairs, const int *port, const int *target,
                                   int group, double *d_records);
size_t gdg_transfer_doubles(int n_pairs, int group);
int gdg_match_taps_from_transfer(const double *records, int n_pairs, int group, size_t blocks, double ridge, int n_taps, int center, double *tap, double *coherence);
/*
 * DELIVERY: the batch calls render at the session rate -- 192 kHz serves the non-linear units -- and the deliverable is a half or a quarter
 * of it (48 kHz from 192, 96 from 192, 44.1 from 88.2 or 176.4).  With a delivery factor in force every encoded port leaves the device at
 * the delivered rate, decimated from the finished float64 rows as they lie on the device: a quarter of the bytes come down and are scattered,
 * and nothing is decimated on a CPU afterwards.
 *   gdg_batch_set_delivery(ctx, factor)                factor 1 (off), 2 or 4
 *   gdg_batch_delivery(ctx)                            the factor in force (1: off, or never set)
 *   gdg_batch_delivery_latency(factor)                 session samples a delivered port lags the render by: 0, 38, 77 (anything else: 0)
 * GDG_ERR_INVALID, with gdg_last_error naming the delivery factor, and the factor in force unchanged: a factor other than 1, 2, 4; a call
 * while a streamed job is open.
 * DEFINITION -- oversampling.Decimate (oversampling/oversampling.go:126-184: a causal anti-aliasing FIR, every factor-th sample, times
 * ATTENUATION_HALF_DECIBEL) without the clip to [-1, 1] the reference's filter applies to its output; the encoders clip.  Factor R; T = 77 taps
 * for R = 2 and 155 for R = 4; h the expanded symmetric table (oversampling.go:239-317, :357-513; gdg_deliver_taps hands it out);
 * A = 0.9440608762859234.  For a port's row x over the WHOLE JOB, with x[n] = 0 for n < 0:
 *   f = h[0] * x[R i]
 *   f = f + (h[k] * x[R i - k])                        for k = 1 .. T - 1, in ascending order
 *   y[i] = A * f
 * every product and every add an IEEE-754 double operation rounded on its own: no fused multiply-add, and the symmetric taps are not folded.
 * A delivered port has samples / R samples and lags the render by (T - 1) / 2 session samples (38 and 77).
 * Known answers: an impulse 1.0 at sample 0 gives y[i] = A * h[R i]; an impulse at sample 1 gives y[i] = A * h[R i - 1] (y[0] = +0.0);
 * silence gives exactly +0.0 everywhere.
 * OFF: factor 1, or never set.  Off, no launch, allocation, buffer or byte differs from a context that never heard of the call; option
 * stat_batch_device_kib is unchanged.
 * WHERE: gdg_batch_run and gdg_batch_stream_step: every encoded port -- the N chain outputs, master left, master right, metronome, the blends.
 * Each out_bytes buffer is gdg_batch_length() / R * width bytes; a streamed slice of b blocks writes b * 8192 / R samples to each.
 * ORDER: decimate, then the gain (gdg_batch_set_trim, a blend's output gain) times the delivered sample, then the plain or the dithered
 * encoder.  The dither's sample index is the delivered sample's index in the job: (the step's first session sample) / R + i.
 * STATE: the last 154 session samples of every port, kept on the device from step to step and from slice to slice: the bytes do not depend on
 * the window or on how a stream is sliced.  Zeroed when a job starts; freed when the factor returns to 1.
 * WHAT STAYS AT THE SESSION RATE: the float64 rows, the master mix, the meters, the tuner, and EVERY record kind -- report, spectrum,
 * alignment, true peak, fits, Gram, tap fits, transfer: they describe the render.  A delivered file's true peak can differ from the render's
 * record (the filter removes what lies above the new Nyquist frequency and rings); the stand-alone record calls can be run on delivered rows.
 * GDG_ERR_UNSUPPORTED while a factor other than 1 is in force, gdg_last_error naming the delivery factor: gdg_batch_stream_checkpoint,
 * gdg_batch_stream_checkpoint_size and the resume calls (the history is not in the version-1 container, as the blend history is not);
 * gdg_batch_run_shard, gdg_batch_stream_open_shard, gdg_batch_stream_step_shard; gdg_batch_finish_master, gdg_batch_finish_master_slice.
 * Configuration, like gdg_batch_set_trim: it holds from the next batch call on, survives batch calls and is part of no blob.
 * The operation on its own:
 *   gdg_deliver_rows(ctx, rows, n_rows, samples, factor, history, out)                                   host buffers, blocking
 *   gdg_deliver_rows_device(ctx, d_rows, row_stride, n_rows, samples, factor, d_history, d_out, out_stride)   enqueued on gdg_ctx_stream
 *                                                      rows: [n_rows][samples] (device: row r at d_rows + r * row_stride); out:
 *                                                      [n_rows][samples / factor] (device: out_stride apart).  samples: any positive
 *                                                      multiple of factor.  history: NULL (zeros in front of sample 0) or [n_rows][154]
 *                                                      doubles, the session samples in front of the call, the newest last; read before and
 *                                                      written after (the call's last 154 samples; a call of fewer moves the old ones up),
 *                                                      so consecutive calls continue a stream.  Factor 1 copies.  Nothing outside
 *                                                      [row, row + samples / factor) of out is written.
 *   gdg_deliver_taps(factor, taps, capacity)           the expanded table h: writes min(T, capacity) doubles (taps may be NULL), returns T
 *                                                      (0 for a factor without a filter); pure host arithmetic
 */
int gdg_batch_set_delivery(gdg_ctx *ctx, int factor);
int gdg_batch_delivery(const gdg_ctx *ctx);
int gdg_batch_delivery_latency(int factor);
int gdg_deliver_rows(gdg_ctx *ctx, const double *rows, int n_rows, size_t samples, int factor, double *history, double *out);
int gdg_deliver_rows_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, int factor, double *d_history, double *d_out,
                            size_t out_stride);
int gdg_deliver_taps(int factor, double *taps, int capacity);
/*
 * DELIVERY, a rational ratio behind the factor: 44.1 kHz from a 48, 96 or 192 kHz session, 48 kHz from 44.1 or 88.2.  Delivery is two stages
 * in series in front of the untouched encoders: the integer factor R above (1, 2 or 4), then a ratio L / M (up / down) applied to what the
 * factor leaves, the INTERMEDIATE rows at rate / R.  192 kHz -> 44.1: factor 4, ratio 147/160; 96 -> 44.1: 2, 147/160; 48 -> 44.1: 1, 147/160;
 * 88.2 -> 48: 2, 160/147.  The long anti-aliasing work at the full rate stays with the factor's filter; the ratio stage runs on a half or a
 * quarter of the data with about 70 taps per output.  resample.Time of the reference (a six-point Lanczos interpolation without an
 * anti-aliasing filter) is right for bringing a file up to the session rate and wrong for going down, so this stage has a definition of its own.
 * (The calls of this block are named gdg_batch_out_* and gdg_out_ratio_*: the census of the factor stage's exports is taken by the word
 * "deliver", and stays as it is.)
 *   gdg_batch_set_out_ratio(ctx, factor, up, down)   holds from the next batch call on; gdg_batch_set_delivery(ctx, factor) means up / down = 1 / 1
 *   gdg_batch_out_ratio(ctx, &up, &down)             the ratio in force (1 / 1: none); gdg_batch_delivery keeps returning the factor
 *   gdg_batch_out_samples(factor, up, down, first, count)   the delivered samples the session samples [first, first + count) produce (both
 *                                                      multiples of factor; 0 for anything inadmissible): what a caller sizes out_bytes with, per
 *                                                      job (first 0, count gdg_batch_length()) and per streamed slice (first = the session samples
 *                                                      of the slices before).  Pure host arithmetic, 64-bit integers
 *   gdg_batch_out_ratio_latency(factor, up, down) session samples a delivered port lags the render by: gdg_batch_delivery_latency(R) + R T / 2
 * ADMISSIBLE RATIOS: gcd(L, M) = 1, 1 <= L <= 160, 1 <= M <= 320, M <= 2 L and L <= 2 M; 1/1 means no ratio stage.  The caller reduces the
 * ratio: an unreduced pair is refused, naming the reduced one.  GDG_ERR_INVALID, gdg_last_error naming the delivery ratio, the factor and the
 * ratio in force unchanged: an inadmissible factor or ratio, an unreduced ratio, a call while a streamed job is open.
 * TAPS PER PHASE: T = 2 * ceil(32 * max(1, M / L)), in integers: 70 for 147/160, 64 for 160/147, at most 128.
 * PROTOTYPE: g[m], m = 0 .. L T - 1, centre c = L T / 2, u = m - c:
 *   g[m] = L * 2 fc * sinc(2 fc u) * I0(beta * sqrt(1 - (u / c)^2)) / I0(beta)
 * fc = 0.5 / max(L, M) (the cut-off is the Nyquist frequency of the lower of the two rates), beta = 10, sinc(v) = sin(pi v) / (pi v).  Computed
 * once on the host in float64 when the ratio is set, stored as tap[p][t] = g[p + t L].
 * OUTPUT: for an intermediate row x over the WHOLE JOB with x[k] = 0 for k < 0, output n has b = floor(n M / L) and p = (n M) mod L, and
 *   f = tap[p][0] * x[b]
 *   f = f + (tap[p][t] * x[b - t])                     for t = 1 .. T - 1, in ascending order
 *   y[n] = f
 * every product and every add an IEEE-754 double operation rounded on its own; no attenuation constant and no clip (the encoders clip).  The
 * filter is causal: output n needs nothing beyond x[b].
 * COUNTS: the intermediate samples [s0, s1) produce the outputs ceil(s0 L / M) <= n < ceil(s1 L / M); a job of S session samples has
 * ceil((S / R) * L / M) delivered samples per port.  64-bit integers throughout, no floating point.
 * LATENCY: the ratio stage lags by T / 2 intermediate samples, exactly (the centre is on the grid): a delivered port lags the render by
 * gdg_batch_delivery_latency(R) + R * T / 2 session samples.
 * Known answers: an impulse 1.0 at intermediate sample 0 gives y[n] = g[n M] while n M < L T, and +0.0 after; silence gives exactly +0.0; after
 * T samples of 1.0 every output is its phase's tap sum, within 3e-6 of 1 for 147/160, 160/147, 2/3, 3/2 and 1/2.
 * ORDER: factor, ratio, then the trim or blend gain, then the plain or the dithered encoder.  The dither's index is the delivered sample's
 * index n in the job.
 * WHERE: gdg_batch_run writes gdg_batch_out_samples(R, L, M, 0, gdg_batch_length()) samples to each out_bytes buffer; a streamed slice of b
 * blocks behind `done` session samples writes gdg_batch_out_samples(R, L, M, done, b * 8192) samples to each -- the count differs from slice
 * to slice (8192 * 147 / 160 = 7526.4), and the slices' counts sum to the job's.
 * STATE: beside the factor's 154 session samples, GDG_DELIVER_RATIO_HISTORY = 127 intermediate samples of every port, kept from step to step and
 * from slice to slice, zeroed when a job starts, freed when delivery returns to off.  The bytes do not depend on the window or the slicing.
 * What stays at the session rate, and off (never set, or factor 1 with 1/1): as above.
 * GDG_ERR_UNSUPPORTED while a ratio other than 1/1 is in force, gdg_last_error naming the delivery ratio: the checkpoint and resume calls (the
 * histories are not in the version-1 container), the shard calls, gdg_batch_finish_master and gdg_batch_finish_master_slice.
 * The ratio stage on its own:
 *   gdg_out_ratio_rows(ctx, rows, n_rows, samples, up, down, first, history, out, out_capacity)      host buffers, blocking
 *   gdg_out_ratio_rows_device(ctx, d_rows, row_stride, n_rows, samples, up, down, first, d_history, d_out, out_stride)   enqueued on gdg_ctx_stream
 *                                                      rows: [n_rows][samples] intermediate samples, the job's [first, first + samples) (device:
 *                                                      row r at d_rows + r * row_stride); out: row r at out + r * out_capacity (device:
 *                                                      out_stride), its first ceil((first + samples) L / M) - ceil(first L / M) samples written
 *                                                      and nothing else; a capacity or stride below that count is refused.  history: NULL
 *                                                      (zeros in front of the call) or [n_rows][127] doubles, the newest last, read before and
 *                                                      written after (a call of fewer samples moves the old ones up), so that consecutive calls
 *                                                      with advancing `first` continue a stream.  1/1 copies.
 *   gdg_out_ratio_taps(up, down, taps, capacity)   the table tap[L][T]: writes min(L T, capacity) doubles (taps may be NULL), returns L T
 *                                                      (0 for an inadmissible ratio and for 1/1); pure host arithmetic
 */
int gdg_batch_set_out_ratio(gdg_ctx *ctx, int factor, int up, int down);
int gdg_batch_out_ratio(const gdg_ctx *ctx, int *up, int *down);
size_t gdg_batch_out_samples(int factor, int up, int down, size_t first, size_t count);
int gdg_batch_out_ratio_latency(int factor, int up, int down);
int gdg_out_ratio_taps(int up, int down, double *taps, int capacity);
int gdg_out_ratio_rows(gdg_ctx *ctx, const double *rows, int n_rows, size_t samples, int up, int down, size_t first, double *history, double *out, size_t out_capacity);
int gdg_out_ratio_rows_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, int up, int down, size_t first, double *d_history,
                                  double *d_out, size_t out_stride);
/*
 * DELIVERED RECORDS: every record kind above describes the session-rate render.  With a delivery in force what a job writes is something else
 * -- rows passed through the factor's decimator and perhaps the ratio stage -- and a band-limiting filter moves peaks: a file "normalised to
 * -1 dBTP" from the render's records can come out above it.  This record measures the rows the encoders read: the delivered rows, in the
 * blocks the delivery gives them, with a true peak defined over the whole delivered stream -- a short history goes from step to step, as the
 * delivery stages themselves keep one -- so that no interval at a block boundary is left out.
 * (The calls of this block are named gdg_block_out_rows, gdg_batch_out_records* and gdg_trim_from_out_records: the census of the factor
 * stage's exports is taken by the word "deliver", and stays as it is.)
 */
typedef struct {
    double   true_peak;   /* max of |x[i]| over the block's samples and of |v_p[n]| over the points that complete in it */
    double   peak;        /* max of |x[i]| over the block's samples */
    double   sum_sq;      /* sum of x[i]^2 over the block's samples, in block_stats_kernel's order at L = the block's length */
    int32_t  position;    /* 4 (n - o) + p of the first point that attains true_peak, o = the block's first delivered sample; p = 0 for a sample;
                             can be as low as -47; 0 when true_peak == 0 */
    uint32_t peak_index;  /* i - o of the first sample that attains peak */
    uint32_t overs;       /* interpolated points (p = 1, 2, 3) completing in the block with |v| > 1 */
    uint32_t clipped;     /* samples of the block with |x| > 1 */
} gdg_block_delivered;    /* 40 bytes, little-endian, no padding */
/*
 * BLOCKS: delivered block k of a port is the delivered samples N(8192 k) <= n < N(8192 (k + 1)) with N(s) = gdg_batch_out_samples(factor, up,
 * down, 0, s): exactly the samples session block k produces.  Its length is 8192 / R behind a factor alone, one of two neighbouring counts
 * behind a ratio (8192 / 4 * 147 / 160 = 1881.6: 1881 or 1882), between 1024 and 16384 over the admissible ratios.  One record per port and
 * session block: [ports][blocks], the shape of every other record kind.  With no delivery in force the blocks are the 8192-sample session
 * blocks: a seamless true peak of a session-rate job.
 * THE SAMPLES' PART (peak, peak_index, sum_sq, clipped) is gdg_block_stats' definition and order at L = the block's length: thread t of 256
 * takes the pairs t, t + 256, .. in ascending order into one running sum; a wave reduces by the tree + 32, + 16 .. + 1; the four wave sums are
 * added in wave order; every square and add is an IEEE-754 double operation rounded on its own.  A non-finite sample is taken as 0 everywhere
 * in this record (gdg_block_stats.nonfinite already counts them at the session rate).
 * THE INTERPOLATED PART uses the taps of gdg_true_peak_taps (H = 12, three phases of 24): for interval n, between the samples n and n + 1,
 *   v_p[n] = sum_j x[n + j] * h_p[j],  j = -H+1 .. H                     the value at position n + p/4
 * accumulated from 0.0 in ascending j, every product and add rounded on its own.  Interval n belongs to the block that holds sample n + 12,
 * the last sample it reads: a block needs the 23 samples in front of it and nothing behind it, and every interval of the stream belongs to
 * exactly one block.  In front of a stream stand zeros, so the twelve intervals that end with the first block's first twelve samples are
 * evaluated over them (the band-limited onset of the stream).  The last 12 intervals of a job -- the ones that would read beyond its last
 * sample -- are the only ones never looked at.  "Better" is the greater magnitude, then the lower signed position.
 * A record is a function of the block's samples and the 23 in front of them alone: not of the window, the slicing, the row or the grid.
 * Known answers: silence gives all zeros.  An impulse of 1.0 at o + 100 gives true_peak 1.0, position 400 and overs 0.  Two samples of 0.8
 * at o - 1 and o (the last of block k - 1 and the first of block k) and nothing else: block k has peak 0.8, true_peak = 0.8 (h_2[0] + h_2[1])
 * ~ 1.0141 (the two centre taps of the half-way phase, each 0.633825), position -2 and overs 1; block k - 1 has true_peak 0.8; and
 * gdg_block_true_peak_rows on either block alone reports 0.8 -- the hole this record closes.
 *   gdg_block_out_rows(ctx, rows, n_rows, samples, span, n_blocks, history, records)
 *                                                      n_rows host rows of `samples` float64 each, cut into n_blocks blocks by span[0 .. n_blocks]:
 *                                                      ascending, span[0] = 0, span[n_blocks] = samples, every length 1 to 16384 -- anything
 *                                                      else is refused.  records: [n_rows][n_blocks], row-major.  history: NULL (zeros stand in
 *                                                      front, nothing is kept) or [n_rows][23] doubles, the newest last, read before and
 *                                                      written after (a call of fewer than 23 samples moves the old ones up): two calls that
 *                                                      continue each other through it give the records of the one call
 *   gdg_block_out_rows_device(ctx, d_rows, row_stride, n_rows, samples, span, n_blocks, d_history, d_records)
 *                                                      the same on device memory, enqueued on gdg_ctx_stream: row r at d_rows + r * row_stride
 *                                                      (row_stride >= samples, any 8-byte alignment); span stays a host array; no sample
 *                                                      outside [row, row + samples) is read
 *   gdg_batch_out_records_enable(ctx, enable)          from the next batch call on, gdg_batch_run and gdg_batch_stream_step keep the records of
 *                                                      every encoded port -- chain outputs, master left and right, metronome, blends, in the
 *                                                      encoders' order -- taken from the rows the encoders read, BEFORE the trim or blend gain (a
 *                                                      gain g scales true_peak and peak by |g| up to one rounding).  The delivery stages run
 *                                                      whether or not the call passes output buffers.  State: 23 doubles per port, zeroed by a
 *                                                      job's first slice, kept from step to step and slice to slice, freed when the switch goes
 *                                                      off.  Off (the default): no launch, buffer or byte differs.  GDG_ERR_INVALID while a
 *                                                      streamed job is open.  Configuration: part of no blob
 *   gdg_batch_out_records(ctx, records, capacity, &ports, &blocks)
 *                                                      the records of the LAST COMPLETED batch call, [ports][blocks] row-major; records == NULL:
 *                                                      the counts only.  GDG_ERR_INVALID when capacity < ports * blocks or there are none
 *   gdg_trim_from_out_records(records, ports, blocks, target, max_gain, gain)
 *                                                      gdg_trim_from_true_peak's rule on this record's true_peak; ports and blocks are at
 *                                                      least 1 (GDG_ERR_INVALID otherwise, as for NULL records or gain)
 * The records come down with each step's own download, behind the transfer records.  GDG_ERR_UNSUPPORTED while the switch is on,
 * gdg_last_error naming gdg_batch_out_records_enable: the checkpoint and resume calls (the history is not in the version-1 container), the
 * shard calls, gdg_batch_finish_master and gdg_batch_finish_master_slice.
 */
#define GDG_OUT_RECORDS_HISTORY 23
#define GDG_OUT_RECORDS_MAX_BLOCK 16384
int gdg_block_out_rows(gdg_ctx *ctx, const double *const *rows, int n_rows, size_t samples, const size_t *span, size_t n_blocks, double *history, gdg_block_delivered *records);
int gdg_block_out_rows_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, const size_t *span, size_t n_blocks, double *d_history,
                              gdg_block_delivered *d_records);
int gdg_batch_out_records_enable(gdg_ctx *ctx, int enable);
int gdg_batch_out_records(gdg_ctx *ctx, gdg_block_delivered *records, size_t capacity, int *ports, size_t *blocks);
int gdg_trim_from_out_records(const gdg_block_delivered *records, int ports, size_t blocks, double target, double max_gain, double *gain);
/*
 * LOUDNESS: K-weighted loudness after ITU-R BS.1770.  Rigs with equal peaks differ by many dB in loudness; "bring these renders to -18 LUFS"
 * needs a record of its own.  BS.1770 gates 400 ms blocks on a 100 ms hop, and a hop -- H = rate / 10 samples: 19200, 9600, 4800, 4410 -- neither
 * divides the 8192-sample block nor is divided by it: the records are kept per HOP, not per block, on a path of their own beside the block
 * records.  A rate that is not a multiple of 10, or below 8000, is refused.
 * K-WEIGHTING: two biquads in series at the session rate fs in float64, their coefficients made on the host at every rate by the same
 * formulas.  With K = tan(pi f0 / fs) and a0 = 1 + K/Q + K^2:
 *   shelf      f0 = 1681.974450955533  Q = 0.7071752369554196  G = 3.999843853973347 dB:  Vh = 10^(G/20), Vb = Vh^0.4996667741545416,
 *              b0 = (Vh + Vb K/Q + K^2) / a0   b1 = 2 (K^2 - Vh) / a0   b2 = (Vh - Vb K/Q + K^2) / a0   a1 = 2 (K^2 - 1) / a0   a2 = (1 - K/Q + K^2) / a0
 *   high-pass  f0 = 38.13547087602444  Q = 0.5003270373238773:  b = (1, -2, 1), a1 and a2 as above from this stage's f0 and Q
 * gdg_loudness_coefficients(rate, out) hands out shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2; at 48000 they are the table printed in BS.1770
 * to 3e-11.
 * RECURRENCE, per sample x (non-finite: 0) from the states s0 = s1 = q0 = q1 = 0 in front of the job, every product, sum and difference an
 * IEEE-754 double operation rounded on its own:
 *   y1 = b0 x + s0        s0 = ((b1 x) - (a1 y1)) + s1        s1 = (b2 x) - (a2 y1)                       the shelf, transposed direct form II
 *   y  = y1 + q0          q0 = q0 + (q1 - (beta y))           q1 = q1 - (alpha y)                          the high-pass
 * with alpha = 4 K^2 / a0 (= 1 + a1 + a2) and beta = (2 K/Q + 4 K^2) / a0 (= 2 + a1) of the high-pass: the same transfer function as
 * b = (1, -2, 1) over (1, a1, a2), in the states q0 = t0 and q1 = t0 + t1 of its transposed direct form II.  The poles lie within 0.3 % of z = 1,
 * where the direct form loses five digits to the roundings of a1 and a2; this one does not.
 * HOP RECORD: for port p and hop h one double, the sum of y[n]^2 over h H <= n < (h + 1) H, n counted from the job's start.  A hop that the job's
 * end cuts is never emitted.  gdg_loudness_hops(rate, first, count) = floor((first + count) / H) - floor(first / H) is the number of hops that
 * complete in the samples [first, first + count): slices and stand-alone calls size their buffers with it, as they do with
 * gdg_batch_out_samples.  A silent port gives exactly +0.0.
 * ORDER: the filter is recursive, so the order of evaluation is part of the definition.  Every 8192-sample block counted from the job's start
 * is a tile of 256 chunks of 32 samples.  Chunk t run from zero states (chunk 0: from the tile's incoming states) ends in the states f_t; then
 * v_t = f_t and, for k = 0 .. 7 in turn, v_t = (P_k v_(t - 2^k)) + v_t for every t >= 2^k at once, P_k = A^(32 * 2^k) in float64 by repeated
 * squaring of A, the 4 x 4 map of the states at x = 0 (row i of P_k v: ((m0 v0 + m1 v1) + m2 v2) + m3 v3).  Chunk t is then run again from
 * v_(t - 1), which gives y; v_255 goes into the next tile.  The squares are summed sequentially in cells of 64 samples counted from the hop's
 * start (the last cell of a hop of 4410 has 58), the cells sequentially in ascending order.  So a hop's 64 bits are a function of the job's
 * samples and the rate alone: not of the window, of how a streamed job is sliced, or of whether outputs are written.  Against the recurrence run
 * sequentially in 80-bit arithmetic a hop differs by less than 1e-9 of its value (DESIGN.md 4.12l has the measured figures).
 * STATE per port, GDG_LOUDNESS_STATE_DOUBLES = 7: s0, s1, q0, q1, the open cell's sum, the open hop's sum, the position (samples seen, exact).
 * Known answers (BS.1770, EBU Tech 3341; their tolerance is 0.1 LU): a full-scale 997 Hz sine on one channel reads -3.01 LUFS at 44100, 48000
 * and 192000; a 1 kHz sine at -23 dBFS on left and right reads -23.0 LUFS; -36 dBFS for 10 s, -23 dBFS for 60 s, -36 dBFS for 10 s reads
 * -23.0 LUFS; silence reads -inf.
 *   gdg_loudness_rows(ctx, rows, row_stride, n_rows, first, count, rate, state_in, state_out, records, capacity)      host buffers, blocking
 *   gdg_loudness_rows_device(ctx, d_rows, row_stride, n_rows, first, count, rate, d_state_in, d_state_out, d_records, records_stride)
 *                                                      enqueued on gdg_ctx_stream.  Row r at rows + r * row_stride holds the job's samples
 *                                                      [first, first + count); its gdg_loudness_hops(rate, first, count) records go to
 *                                                      records + r * capacity (records_stride), and nothing else is written; less room is
 *                                                      refused.  state_in == NULL starts a stream, and then `first` must be 0; a continuing
 *                                                      call passes the [n_rows][7] doubles the call before wrote to state_out and begins at a
 *                                                      multiple of 8192 samples -- any other `first` is refused, and so (host form) is a state
 *                                                      whose position is not `first`.  state_out may be NULL, and may be state_in
 *   gdg_batch_loudness_enable(ctx, enable)             from the next batch call on, gdg_batch_run and gdg_batch_stream_step keep the hop records
 *                                                      of every encoded port -- chain outputs, master left and right, metronome, blends --
 *                                                      taken from the float64 rows at the session rate, where the block statistics take theirs:
 *                                                      in front of delivery, trim and blend gain.  The kernel also runs in a call that passes
 *                                                      no output buffers.  State and records stay in device buffers of their own: zeroed by a
 *                                                      job's first slice, kept from step to step and slice to slice, freed when the switch goes
 *                                                      off, when stat_batch_device_kib is that of a context that never heard of it.  Off (the
 *                                                      default): no launch, buffer or byte differs.  GDG_ERR_INVALID while a streamed job is
 *                                                      open.  Configuration: part of no blob
 *   gdg_batch_loudness(ctx, records, capacity, &ports, &hops)
 *                                                      the records of the LAST COMPLETED batch call or slice, [ports][hops] row-major, hops =
 *                                                      gdg_loudness_hops(rate, slice's first sample, its samples); downloaded by this call.
 *                                                      records == NULL: the counts only.  GDG_ERR_INVALID when capacity < ports * hops or there
 *                                                      are none
 *   gdg_loudness_from_hops(records, n_ports, n_hops, rate, port, weight, n, &integrated, &momentary_max, &short_term_max)
 *                                                      pure float64 on the host, no context: the programme is the n listed ports with BS.1770's
 *                                                      channel weights (weight == NULL: every one 1.0).  POWER over a hop is the weighted sum of
 *                                                      the ports' hop sums / H.  A 400 ms block is four consecutive hops, block j = hops j ..
 *                                                      j + 3, its power their mean.  integrated = -0.691 + 10 log10(mean of the blocks above
 *                                                      -70 LUFS and above -10 LU relative to the mean of those); momentary_max the largest
 *                                                      block, short_term_max the largest mean of 30 consecutive hops, each as LUFS.  With no
 *                                                      block above the absolute gate: -inf, and success.  Any of the three may be NULL
 *   gdg_trim_from_loudness(records, n_ports, n_hops, rate, target_lufs, ceiling_dbtp, true_peak, blocks, gain, capped)
 *                                                      one gain per port, 10^((target_lufs - L) / 20) with L the port's own integrated loudness
 *                                                      at weight 1; 1.0 for a port that has none.  With true_peak ([n_ports][blocks], NULL: no
 *                                                      cap) a gain that would carry the port's largest true peak over 10^(ceiling_dbtp / 20) is
 *                                                      capped by gdg_trim_from_true_peak's rule -- min(ceiling / peak, gain) -- and capped[p]
 *                                                      (may be NULL) is 1 for such a port, 0 otherwise
 * GDG_ERR_UNSUPPORTED while the switch is on, gdg_last_error naming gdg_batch_loudness_enable: the checkpoint and resume calls (the state is not
 * in the version-1 container), the shard calls, gdg_batch_finish_master and gdg_batch_finish_master_slice.  With a delivery factor in force the
 * file is quieter than the render's record by the decimator's attenuation; a record at the delivered rate is out of scope.
 */
#define GDG_LOUDNESS_STATE_DOUBLES 7
#define GDG_LOUDNESS_TILE 8192
int gdg_loudness_coefficients(uint32_t rate, double *out);
size_t gdg_loudness_hops(uint32_t rate, size_t first, size_t count);
int gdg_loudness_rows(gdg_ctx *ctx, const double *rows, size_t row_stride, int n_rows, size_t first, size_t count, uint32_t rate, const double *state_in, double *state_out,
                      double *records, size_t capacity);
int gdg_loudness_rows_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t first, size_t count, uint32_t rate, const double *d_state_in,
                             double *d_state_out, double *d_records, size_t records_stride);
int gdg_batch_loudness_enable(gdg_ctx *ctx, int enable);
int gdg_batch_loudness(gdg_ctx *ctx, double *records, size_t capacity, int *ports, size_t *hops);
int gdg_loudness_from_hops(const double *records, int n_ports, size_t n_hops, uint32_t rate, const int *port, const double *weight, int n, double *integrated,
                           double *momentary_max, double *short_term_max);
int gdg_trim_from_loudness(const double *records, int n_ports, size_t n_hops, uint32_t rate, double target_lufs, double ceiling_dbtp, const gdg_block_true_peak *true_peak,
                           size_t blocks, double *gain, int *capped);

#ifdef __cplusplus


}
#endif
#endif
