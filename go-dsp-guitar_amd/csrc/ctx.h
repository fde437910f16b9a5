/*
 * ctx.h -- what the host side of libgdg.so shares between its source files: the context, the per-unit records, the plan's step
 * descriptors, the small helpers every entry point uses (fail / enter / HIP_TRY), the copy-worker pool and the profiling scope, and
 * the handful of functions one file offers the others.  Not part of the ABI (include/gdg.h is); everything declared here has hidden
 * visibility: libgdg.so exports the gdg_* entry points and nothing else.
 *
 *   api_ctx.cpp         context life cycle, options, NUMA placement, units and chains, profiling, device-memory helpers, stand-alone FFT
 *   api_plan.cpp        per-unit constants (prepare_unit), scan tables, IR spectra / delay lines (prepare_fir), the launch plan (build_plan)
 *   api_process.cpp     parameter patches, process_rows (the launch sequence of a call), the process entry points, staging + copy workers
 *   api_tuner_spat.cpp  tuner and spatializer glue
 *   api_io.cpp          wave codecs, resample.Time, level meters, power-amp compilation, metronome
 *   api_batch.cpp       the batch run (gdg_batch_run, its sharded form, the streamed forms of both, the master mix of a job and of a slice)
 *   api_state.cpp       channel state saved into / loaded from a blob (gdg_state_*; the copies: state.hip)
 *   api_checkpoint.cpp  a streamed batch run checkpointed into a container and resumed from it (gdg_batch_stream_checkpoint / _resume; the digest: state.hip)
 *   api_loudness.cpp    the loudness records (gdg_loudness_*, gdg_batch_loudness*, gdg_trim_from_loudness; the kernel: loudness.hip)
 */
#ifndef GDG_CTX_H
#define GDG_CTX_H

#include "../../include/gdg.h"
#include "gdg_internal.h"
#include "aa_taps.h"
#include "deliver.h"
#include "go_consts.h"
#include "notes.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <unistd.h>
#include <pthread.h>
#include <sched.h>
#include <sys/syscall.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <memory>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "arena.h"
#include "batch_sources.h"
#include "dither.h"
#include "report_sections.h"
#include "trim.h"
#include "blend.h"
#include "loudness.h"

#define NUM_FILTERS 8

#pragma GCC visibility push(hidden)

/* DevArena: arena.h over the HIP runtime */
struct HipArenaBackend {
    using err_t = hipError_t;
    using stream_t = hipStream_t;
    static err_t ok() { return hipSuccess; }
    static err_t malloc(void **p, size_t n) { return hipMalloc(p, n); }
    static void free(void *p) { (void)hipFree(p); }
    static err_t fill_zero(void *p, size_t n, stream_t st) { return hipMemsetAsync(p, 0, n, st); }
    static err_t wait(stream_t st) { return hipStreamSynchronize(st); }
    static void wait_device() { (void)hipDeviceSynchronize(); }
};
using DevArena = ArenaT<HipArenaBackend>;

/* IR spectra of one (taps, partition size) pair; power amps with identical composite filters share one copy in HBM
 * (the MAC then streams it from L2 / MALL for all but the first channel: SURVEY.md 8d, d < 1) */
struct SharedSpectra {
    std::vector<double> taps;
    int P = 0, K = 0, hop = 0;
    double2 *d_H = nullptr;
    DevArena *arena = nullptr;
    ~SharedSpectra() { if (d_H && arena) arena->release(d_H); }
};

struct Unit {
    bool alive = false;
    int type = 0, channel = 0;
    int32_t params[GDG_MAX_PARAMS] = { 0 };
    /* segment state */
    double *d_ds = nullptr;
    int *d_is = nullptr;
    double *d_hist = nullptr;
    size_t hist_len = 0;
    long long hist_key = -1;          /* what the current history layout was built for */
    int os_frames[2] = { -1, -1 };    /* frame size the 2x / 4x oversampler last saw */
    int bp_half_order = -1;
    bool ran = false;                 /* a plan has laid the unit out (prepare_unit): a state save records it, a unit that never ran saves as fresh */
    /* FIR */
    std::vector<double> taps;
    bool fir_dirty = true;
    bool fir_live = false;
    int fir_P = 0, fir_K = 0, fir_hop = 0;     /* transform half size (power of two), partitions, samples per frame */
    int fir_R = 0;                             /* delay-line ring slots: fir_K + window - 1 */
    uint32_t fir_sr = 0;
    double *d_prev = nullptr;
    double2 *d_fdl = nullptr, *d_Y = nullptr;
    std::shared_ptr<SharedSpectra> H;
    int *d_pos = nullptr;                      /* [4]: the frame counter, the stamp of the sums made ahead (gdg_internal.h) */
    double2 *d_acc = nullptr;                  /* [T][P] sums made ahead of the next T frames (Shape FUSED_AHEAD) */
    size_t acc_bytes = 0;
};

struct Slot { int handle; bool bypass; };
#define GDG_WAVE_STEPS 64             /* segment steps of a plan that can run as WAVE launches (a chain with more power amps than that walks) */
#define GDG_WAVE_GROUPS 16            /* = the most channel groups of a call (every group's launch of a step draws its own tickets) */

/* How a step is launched.  decide_shapes (api_plan.cpp) picks one per call kind when the plan is built; process_rows dispatches by it. */
enum class Shape : unsigned char {
    SKIP,               /* not launched: the oversampled shaper's launch behind it runs its compressor (OS_TILES_PREFIX) */
    GENERAL,            /* segment: the general kernel, one frame, a workgroup per channel */
    GENERAL_AHEAD,      /* ... and extra workgroups that make the wet paths of later steps' reverbs (seg.hip REVERB_AHEAD) */
    SEGF,               /* segment: the two-per-CU kernel (seg.hip SEG_FAST) */
    SEGT,               /* segment: a channel's frame on two workgroups (seg.hip SEG_TILE) */
    WAVE, SEGF_WAVE,    /* window: a workgroup per frame and channel, the frames meeting unit by unit (seg.hip WAVE) */
    WALK, SEGF_WALK,    /* window: a workgroup per channel walks the frames */
    OS_TILES,           /* one oversampled shaper per channel as a launch of its own (seg.hip os_tiles_kernel) */
    OS_TILES_PREFIX,    /* ... whose workgroups also run the lone compressor of the step in front */
    FUSED,              /* power amp: multiply-accumulate inside the inverse transform's kernel */
    SPLIT,              /* power amp: the bin-tiled multiply-accumulate, then the inverse transform */
    SPLIT_PREMAC,       /* ... whose terms k >= 1 the previous call sums ahead of the frame (premac) */
    FIR_WINDOW,         /* power amp in a window (fir.hip, time blocking) */
    FUSED_AHEAD,        /* FUSED, continuing the sums a pass at the call's start made for the next T frames (fir_ahead_kernel) */
};
static inline const char *shape_name(Shape s) {
    static const char *const names[] = { "SKIP", "GENERAL", "GENERAL_AHEAD", "SEGF", "SEGT", "WAVE", "SEGF_WAVE", "WALK", "SEGF_WALK",
                                         "OS_TILES", "OS_TILES_PREFIX", "FUSED", "SPLIT", "SPLIT_PREMAC", "FIR_WINDOW",
                                         "FUSED_AHEAD" };
    return names[(int)s];
}

struct StepDesc {
    bool is_fir;
    int n;
    size_t offset;                    /* byte offset of its descriptor array inside the plan blob */
    Shape window = Shape::SKIP;       /* how a window launches it; per-frame calls: runs[g].frame */
    struct Run { int first = 0, n = 0; Shape frame = Shape::SKIP; };
    std::vector<Run> runs;            /* per channel group: (first descriptor, count) and how a per-frame call launches them */
    bool shared_spectra = false;      /* FIR step: some channels read the same IR spectra */
    bool chain_next = false;          /* FIR step whose every channel feeds another power amp next (the following step): that amp's forward
                                       * transform rides on this step's inverse (fir_inv_kernel CHAIN) */
    int premac_lds = 0;               /* FIR step: the LDS its premac launch asks for without using it (decide_shapes) */
    int fir_ahead_T = 0;              /* FIR step: > 0 when some group's launch is FUSED_AHEAD -- the frames one pass ahead serves (decide_shapes) */
    int os_factor = 0;                /* 2 / 4: the step is ONE oversampled shaper per channel, run as a launch of its own (seg.hip os_tiles_kernel) */
    int os_flags = -1;                /* ... and its per-channel flags start here in d_wave */
    int os_arrive = -1;               /* ... its per-channel arrival counters (a compressor step absorbed into the launch, below) */
    int os_prefix_step = -1;          /* ... OS_TILES_PREFIX: the step right in front of it, a lone compressor in every one of its channels */
    int ahead_n = 0;                  /* segment step (one frame per launch): it also makes the wet paths of this many reverbs of LATER steps ... */
    size_t ahead_offset = 0;          /* ... whose indices into the plan's unit array start here in the blob (seg.hip REVERB_AHEAD) */
    int wave_tickets = -1;            /* segment step: first of its GDG_WAVE_GROUPS ticket counters in d_wave (seg.hip, WAVE), -1: none */
};

struct ProfEvent { int kind; hipEvent_t a, b; };
class CopyPool;

/* two pinned host halves of one size, for a transfer that fills one while the other is on the bus: kept from call to call, grown when a
 * call needs more (never shrunk), freed with the context */
struct PinnedHalves {
    unsigned char *half[2] = { nullptr, nullptr };
    size_t cap = 0;
    unsigned char *operator[](size_t h) const { return half[h]; }
    hipError_t grow(gdg_ctx *ctx, size_t bytes);      /* both halves hold at least `bytes` afterwards; what they held is gone when they grew */
    void release();
};

struct gdg_ctx {
    int nch = 0, max_frames = 0, device = 0;
    hipStream_t stream = nullptr;
    mutable std::string err;
    std::vector<Unit> units;
    std::vector<std::vector<Slot>> chains;
    bool dirty = true;
    /* cached plan */
    int plan_frames = 0;
    uint32_t plan_sr = 0;
    const double *plan_in = nullptr;
    double *plan_out = nullptr;
    std::vector<int> plan_active, all_channels;
    int plan_stride = 0, plan_stride_out = 0;
    bool plan_by_channel = false;
    std::vector<StepDesc> steps;
    std::vector<int> plan_unit_slot;           /* unit handle -> index of its descriptor in the plan's array of gdg_seg_unit, -1: not in the plan */
    std::vector<char> plan_unit_fast;          /* ... and whether its segment runs on the two-per-CU kernel (scan tables for 16-sample chunks) */
    std::vector<char> plan_unit_fast_ok;       /* ... and whether the unit itself could (segf_unit_ok at plan time): a change of that rebuilds the plan */
    bool seg_fast = true;                      /* GDG_SEG_FAST=0: every segment on the general kernel (A/B measurements, bit-identity tests) */
    int seg_fast_min = 128;                    /* GDG_SEG_FAST_MIN: fewest channels of a call that take the two-per-CU kernel.  Per-frame calls of up to a chip's
                                                * worth of channels finish a frame 1-3 % sooner on the general kernel (one round of 1024-thread workgroups; 128
                                                * channels 214 vs 217 us per step, 256: 301 vs 305; profiles/fast_min_ab_r04.txt) -- but windows of few channels
                                                * run a workgroup per frame (WAVE, below), and there twice the frames in flight are worth 7-13 % from 128 channels
                                                * on (W = 16: 96 channels 65.1 vs 63.0 us per frame, 128: 83.1 vs 76.8, 256: 159 vs 137.6; not from 96: per-frame
                                                * calls of 96 channels lose 13 % -- pairs of 512-thread workgroups land on one CU beside the premac).  ONE threshold for both
                                                * kinds of call: the two builds differ in the association of their scans (~1e-16), and a window has to give the
                                                * bits of the same frames called one by one. */
    /* Windows of few channels (seg.hip, WAVE): up to this many channels per launch a window's segment launch puts every FRAME of a channel on a
     * workgroup of its own, the frames meeting unit by unit through counters in HBM -- a GPU's share of the 512-channel job on eight GPUs is 64
     * channels, and one workgroup per channel walking the window leaves 3/4 of the CUs idle (64 channels, W = 16: 417 us per segment launch,
     * 52 of the 77 us per frame).  0: never.  gdg_ctx_set_option("seg_wave_max_channels"), env GDG_SEG_WAVE_MAX. */
    int seg_tile_max = 112;                    /* per-frame calls of up to this many channels: a segment of compressor / shapers / tone stack / cabinet / chorus (/ the mix of a
                                                * reverb made ahead) runs with a channel's frame on TWO workgroups (seg.hip SEG_TILE; same bits) -- as long as the launch's
                                                * workgroups, 2 x channels + the reverbs' extra ones, leave the chip room (decide_shapes) */
    unsigned long long *d_tile_xch = nullptr;  /* what crosses between the two workgroups of a channel: gdg_segt_xch_words() words per descriptor of a launch */
    size_t d_tile_xch_cap = 0;
    bool seg_os_prefix = true;                 /* a lone compressor in front of an oversampled shaper's own launch runs inside that launch in per-frame calls (option seg_os_tiles_prefix) */
    int seg_os_tiles_max = 192;                /* calls of up to this many channels run oversampled shapers as launches of their own, a workgroup per tile
                                                * (option "seg_os_tiles_max_channels"; 0: never) */
    int seg_wave_release_max = 112;            /* ... of segments with a unit whose state leaves the CU through plain stores (flanger, phaser, delay, fuzz, auto-yoy, auto-wah,
                                                * band pass, octaver, noise gate): every hand-off then writes the XCD's L2 back, and from ~128 channels on the walk
                                                * is faster (192 channels 84 vs 66 us per frame, 448: 202 vs 145; profiles/shape_sweep_r06.txt) */
    int seg_wave_max = 448;                    /* W = 16, us per frame, walk -> a workgroup per frame: 64 channels 77 -> 48, 128: 102 -> 77, 256: 146 -> 138, 384: 222 -> 206;
                                                * 512: 259 -> 263 (the walk wins once two workgroups per CU are all busy anyway) */
    int scan_tables_max = 1024;                /* scan tables kept before a plan rebuild drops them all (a caller sweeping a parameter) */
    int pcie_groups_forced = 0;                /* channel groups of the host-buffer calls; 0: by channel count */
    int device_groups_env = 0;                 /* GDG_DEVICE_GROUPS: the debug override of gdg_ctx_set_overlap(0) */
    int copy_threads = 8;                      /* host copy workers of the host-buffer paths (made on first use) */
    int tuner_long = 0;                        /* 1: every analysis through the 262144-point transform pair (A/B, tests) */
    /* NUMA placement of the host paths (option "numa").  The CPU side of a host-buffer call is copying between the CALLER's pageable buffers
     * and the pinned slabs; the GPU's DMA engines reach either socket's memory at PCIe speed.  So the default (2) puts the copy workers and
     * the pinned slabs on the node the caller runs on when they are made; 1 puts them on the device's node (deterministic per GPU, but a
     * caller on the other socket then has every byte read across the socket link: batch run 56 -> 73 ms); 0 leaves both to the scheduler and
     * to hipHostMalloc's default (profiles/host_path_numa_r05.txt: both sockets within 1 % for the batch run and 4 % for the staged call at 2,
     * 30 % / 1 % apart at 1, 0 % / 10 % at 0). */
    int numa_mode = 2;                         /* 0: nothing; 1: the device's node; 2: the node the CALLER runs on when the pool / a slab is made */
    int numa_node = -1;                        /* /sys/bus/pci/devices/<bus id>/numa_node of the device, -1: unknown or a one-node host */
    std::vector<int> numa_cpus;                /* /sys/devices/system/node/node<N>/cpulist */
    std::vector<std::vector<int>> node_cpus;   /* every node's CPUs (mode 2) */
    /* Small shards, per-frame calls (one GPU's share of a job split over several): the convolution's multiply-accumulate is the one kernel
     * of the step that does not depend on the frame for 7/8 of its work -- the terms k = K - 1 .. 1 of Y = sum_k FDL[pos - k] H[k] only need
     * frames that are already in the delay line.  So when a call ends, that part of the NEXT frame's sum is launched on a stream of its own
     * (the "premac": fir_mac_kernel with k_lo = 1 into Y) and runs beside the call's last segment and the next call's first (64 workgroups
     * on a 256-CU chip); the next call's inverse kernel adds the newest term and transforms (fir_inv_kernel FUSED = 4): 2 spectra per channel
     * on the critical path instead of 2 K.  Every multiply-accumulate kernel sums k DESCENDING, so the split sum has the bits of the whole one.
     * The premac is speculative: any library call but a process call drops it (the next call then runs the whole sum). */
    int fir_premac = 1;                        /* option "fir_premac": 0 never */
    int fir_premac_lds = -1;                   /* option "fir_premac_lds_bytes": -1 by channel count (decide_shapes) */
    int fir_premac_min = 384;                  /* fewest partitions (sum of K over a launch's channels) worth it: the two cross-stream hops and the
                                                * three extra spectra of the inverse kernel cost ~20 us per step -- the multiply-accumulate of 48 x 8
                                                * partitions takes that long (16 x 8: 113.7 -> 123.4 us per step with it, 64 x 4 (config 3): 137 -> 141) */
    int fir_premac_min_two = 320;              /* ... with two or more power amps per channel the hops hide twice as much: 40 x 8 partitions per amp 120.6 -> 109.3 us
                                                * per step with it, 32 x 8: 112.4 -> 109.6, 24 x 8: 107.2 -> 108.6 (profiles/premac_loads_ab_r06.txt) */
    hipStream_t premac_stream = nullptr;
    hipEvent_t ev_fir_done = nullptr, ev_premac = nullptr;
    int stat_premac_used = 0;                  /* option "stat_premac_launches_used" (read it; tests): inverse launches that continued sums made ahead
                                                * (saturates at INT_MAX) */
    /* Per-frame calls of many channels (the fused shape): the terms of frame t0 + j with k >= j + 1 only read frames that exist when call t0
     * starts, so ONE pass over H[1 .. K-1] and X[t0-K+1 .. t0-1] makes them for the next T frames (fir_ahead_kernel, on the group's own
     * stream at the call's start), and the inverse kernel of frame t0 + j adds the terms k = j .. 0 (FUSED 5 / 6).  The channels are
     * staggered: call c makes the sums of the channels of phase c mod T (contiguous blocks of n / T of each group), so every call does the
     * same work.  A stamp next to each frame counter on the device holds (frame, epoch) of the sums; the context's epoch moves on whenever
     * anything but a per-frame call of the same plan touches the context (drop_fir_ahead), and a stamp of another epoch is never read. */
    int fir_ahead_frames = 4;                  /* option "fir_ahead_frames": T, 2 .. 4; 0 never */
    int fir_ahead_min = 128;                   /* option "fir_ahead_min_channels": fewest channels of a group's launch (no reverb / flanger chains,
                                                * 128 channels: 126.2 -> 120.0 / 120.1 -> 112.9 us per step, profiles/shape_sweep_r07.txt) */
    int stat_fir_ahead_used = 0;               /* option "stat_fir_ahead_sums_used": channel frames whose inverse kernel continued sums made ahead,
                                                * counted on the device (d_fir_ahead_used; read back when the option is read, saturates at INT_MAX) */
    unsigned long long *d_fir_ahead_used = nullptr;
    unsigned fir_ahead_epoch = 1;              /* 0 is never current: a zeroed stamp is no stamp */
    long long fir_ahead_calls = 0;             /* per-frame calls of this epoch (the phase of the call: fir_ahead_calls mod T) */
    bool premac_valid = false;                 /* Y of every premac step holds the terms k >= 1 of the plan's NEXT frame */
    bool premac_outstanding = false;           /* ... and the context's stream has not been ordered behind that launch yet */
    /* reverbs' wet paths ahead of the frame (seg.hip REVERB_AHEAD): made by extra workgroups of an EARLIER segment launch of the same call */
    int seg_reverb_ahead_max = 72;             /* most channels of a call that does it: 64 channels 156 -> 142 us per step, 96 channels 168 -> 175 (twice the
                                                * workgroups in the first segment launch, and the premac's share of the chip with them); with the premac's
                                                * loads fixed: 64 channels 135.1 -> 125.7, 72: 135.6 -> 134.7, 80: 137.7 -> 140.0, 88: 143.3 -> 147.4 */
    int wave_spin_ms = 1000;                   /* how long a frame waits for its predecessor's counter before the launch gives up (seg.hip wave_spin_expired; d_error[1]) */
    int debug_stall_unit = -1;                 /* test hook: this unit's first counter of a WAVE launch stays away, so that the bounded wait expires */
    int wave_epoch = 0;                        /* a number per WAVE launch (seg.hip: "done" marks carry it) */
    int *d_wave = nullptr;                     /* [GDG_WAVE_STEPS x GDG_WAVE_GROUPS ticket counters | one counter per unit in a segment]: zero between launches */
    size_t d_wave_cap = 0;
    std::vector<int> patch_units;              /* units whose parameters changed since the plan was built: their descriptors are patched in place */
    bool plan_patch = true;                    /* GDG_PLAN_PATCH=0: every parameter change rebuilds the whole plan (A/B measurements) */
    int plan_trace = 0;                        /* GDG_PLAN_TRACE as the last plan read it: 1 a line per plan, 2 also a line per launch (process_rows) */
    std::vector<unsigned char> blob;
    unsigned char *d_blob = nullptr;
    size_t d_blob_cap = 0;
    size_t units_offset = 0;
    /* buffers */
    double *d_w0 = nullptr, *d_w1 = nullptr, *d_scratch = nullptr;
    int window = 1;                            /* frames per channel and call of gdg_process_window_device (time blocking) */
    size_t w_stride = 0;                       /* row stride of d_w0 / d_w1: window * max_frames */
    double *d_stage_in = nullptr, *d_stage_out = nullptr;
    double *h_stage_in = nullptr, *h_stage_out = nullptr;
    int stage_out_stride = 0;         /* > 0: d_stage_out holds one complete block of chain outputs, row c = channel c, this stride */
    int stage_out_frames = 0;         /* ... of this many frames per row */
    int *d_error = nullptr;
    DevArena arena;                   /* per-unit state (see DevArena) */
    std::map<std::vector<double>, double *> scan_tabs;     /* scan tables by their coefficients: one copy per distinct set (scan_tables) */
    std::vector<void *> user_allocs;  /* gdg_device_alloc blocks the caller has not freed (released with the context) */
    /* tables */
    std::map<int, std::pair<double2 *, double2 *>> fir_tables;
    std::multimap<uint64_t, std::weak_ptr<SharedSpectra>> spectra;     /* content hash -> live IR spectra */
    std::vector<std::shared_ptr<SharedSpectra>> pending_ir;           /* spectra allocated by the plan being built, transformed together (flush_ir) */
    bool share_spectra = true;
    /* FIR launch shape.  -1 (default): by channel count -- the fused kernel (one workgroup per channel: multiply-accumulate
     * straight into the inverse transform) needs >= ~128 channels to fill the 256 CUs; below that the multiply-accumulate runs
     * as its own bin-tiled kernel (32 workgroups per channel) followed by the inverse (profiles/channels_sweep_r02.txt).
     * GDG_FIR_FUSED=0 / 1 forces one shape (A/B measurements). */
    int fir_fused = -1;
    int fir_split_max = 192;          /* largest launch (channels) that takes the split shape.  Round 2 measured the two shapes equal at 128 channels
                                       * (220 us per step either way) and set 96; with the sums made ahead of the frame (premac, below) the split shape
                                       * took 207 us there and lost at 192 (252 vs 274), hence 128 until the premac stopped reading through the cache
                                       * (fir.hip, fir_mac_kernel): 128 channels 181 vs 223 fused, 160 215 vs 236, 192 247 vs 257, 208 266 vs 264
                                       * (profiles/shape_sweep_r06.txt, chain d) */
    int fir_split_max_single = 112;   /* ... when the call has ONE power amp per channel: the premac has half as much to hide, and at 128 channels the fused kernel wins
                                       * (one amp: 138.8 split vs 127.1 fused us per step, 96 channels 112 vs 125; profiles/shape_sweep_r06.txt) */
    bool fir_chain = true;            /* GDG_FIR_CHAIN=0: adjacent power amps keep separate launches (A/B measurements, bit-identity tests) */
    double *d_os = nullptr;
    gdg_os_tables os;
    /* profiling */
    unsigned profiling = 0;                  /* bit 0: everything; bit k+1: kernel kind k */
    int prof_every = 1;                      /* gdg_profile_sample: bracket every n-th process call only */
    unsigned long long prof_calls = 0;
    bool prof_now = true;
    bool prof_attach = true;                 /* the fused convolution kernel takes its events itself (kernel timestamps); GDG_PROFILE_ATTACH=0: recorded around it */
    std::vector<ProfEvent> prof;
    std::vector<hipEvent_t> event_pool;
    /* tuner / spatializer */
    double *d_tuner_ring = nullptr;
    int tuner_wp = 0;
    uint32_t tuner_sr = 0;
    double *d_note_freqs = nullptr;
    gdg_tuner_out *d_tuner_out = nullptr, *h_tuner_out = nullptr;      /* results: pinned host memory the kernels write directly (d_ = its device-side address) */
    double2 *d_tuner_work = nullptr, *d_tuner_twn = nullptr, *d_tuner_twm = nullptr;
    int tuner_part_cap = 0;                    /* parts per channel d_tuner_part holds */
    unsigned tuner_seq = 0;                    /* number of the last analysis (every result record carries it: api_tuner_spat.cpp) */
    int tuner_poll = 1;                        /* option tuner_poll_results: the caller polls the records instead of waiting for the stream */
    double2 *d_tuner_part = nullptr;           /* partial sums of a short-lag analysis split over several workgroups per channel */
    std::vector<double> sp_az, sp_dist, sp_level;
    uint32_t sp_hist_sr = 96000;
    double *d_sp_hist = nullptr;               /* [2][nch][sp_hist_len]: read this block / written for the next (sp_hist_cur) */
    int sp_hist_len = 0, sp_hist_cur = 0;
    gdg_spat_chan *d_sp_chan = nullptr;
    double *d_sp_out = nullptr;
    bool sp_dirty = true;
    /* io (wave codecs, resample.Time, level meters) */
    void *d_io[2] = { nullptr, nullptr };
    size_t io_cap[2] = { 0, 0 };
    gdg_meter_rec *d_meter = nullptr;
    int n_meter = 0;
    /* the batch run's PCIe side: two pinned halves, a copy stream and events (ensure_batch_pipe) */
    PinnedHalves h_batch;
    hipStream_t batch_stream = nullptr;
    hipEvent_t batch_ready[2] = { nullptr, nullptr }, batch_moved[2] = { nullptr, nullptr };
    hipEvent_t batch_chunk[2][4] = {};         /* a step's download in four pieces: the scatter into the caller's files starts when the first has landed */
    /* ... and the inputs' way up, step by step: two more pinned halves, a stream, events */
    PinnedHalves h_up;
    hipStream_t batch_up_stream = nullptr;
    hipEvent_t batch_up_ready[2] = { nullptr, nullptr }, batch_begin = nullptr;
    /* the batch run's device buffers, one meaning each for every kind of run (BATCH_INPUTS .. BATCH_SOURCE below): kept from call to call,
     * grown when a slice needs more -- allocating and mapping gigabytes per call cost more than the run (gdg_batch_release frees them) */
    void *batch_dev[18] = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
    size_t batch_dev_cap[18] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    int stat_batch_dev_kib = 0;                /* option "stat_batch_device_kib": the sum of batch_dev_cap in KiB, made when it is read */
    /* a batch job, how far it has come, and per input the source frames handed over: the context's is the streamed run's
     * (gdg_batch_stream_open .. _close); a one-call run describes its own and leaves this one closed */
    struct BatchStreamState {
        bool open = false;
        std::vector<gdg_batch_input> inputs;   /* bytes: non-null = the input has samples (never read) */
        gdg_batch_options opt = {};
        size_t length = 0, pos = 0;            /* samples of every output; samples done */
        std::vector<size_t> brought;           /* source frames [0, brought) of input i have been handed over */
        std::vector<size_t> n_out;             /* samples the input covers in the job: its (resampled) length */
        bool shard = false, run_metro = false; /* opened with gdg_batch_stream_open_shard; ... and this shard runs the job's metronome */
        std::vector<int> source;               /* the source map as it stood when the job was described, when it has a reader (empty otherwise):
                                                * inputs and n_out of a reader are its root's */
    } bstream;
    /* the render report's record kinds (report_sections.h: block statistics, band spectrum, alignment records, true-peak records), one
     * state each: the records of the last completed batch call, [ports][blocks] elements of `elem` bytes (zero bytes are a zeroed record
     * of every kind).  A call that collects a kind (`live`: decided when the call begins, report_begin) fills its store step by step and
     * validates it at its end. */
    struct ReportKind {
        bool live = false, valid = false;
        int ports = 0;
        size_t blocks = 0, elem = 0;
        std::vector<unsigned char> store;
    } report[REPORT_KINDS];
    /* ... and what switches each kind on; configuration, in no blob.  A collecting call takes edges, list and lag as they stood when it
     * began (the *_live copies).  Statistics: gdg_batch_report_enable.  Spectrum: gdg_batch_spectrum_enable (spectrum_bands.h), the edges
     * in force (empty = off) and the 8192 window weights (made with the first use, never with the switch off).  Alignment:
     * gdg_batch_align_enable (align_map.h), the reference list and the lag range in force (empty = off); the finish calls never collect.
     * True peak: gdg_batch_true_peak_enable (true_peak_taps.h). */
    bool report_on = false, tp_on = false;
    std::vector<double> spec_edges, spec_live_edges;
    double *d_spec_win = nullptr;
    std::vector<int> align_ref, align_live_ref;
    int align_lag = 0, align_live_lag = 0;
    /* the source map (gdg_batch_set_sources; batch_sources.h): batch_source[c] = the channel whose input entry channel c reads, empty = every
     * channel its own.  Configuration like report_on: read when a job is described, in no blob. */
    std::vector<int> batch_source;
    /* the dither of the LPCM outputs (gdg_batch_set_dither; dither.h): mode 0 = off, 1 = TPDF; the job-wide index of the context's first
     * channel; the sample index the next gdg_batch_finish_master_slice starts at.  Configuration like the source map: in no blob. */
    int dither_mode = 0;
    uint64_t dither_seed = 0, dither_cursor = 0;
    uint32_t dither_port_base = 0;
    /* the output trim (gdg_batch_set_trim; trim.h): a gain per output port in front of the encoders -- the context's chain outputs, then
     * master left, master right, metronome: nch + 3 entries, the rows of a batch window -- empty = off (never set, or every gain 1.0).  The
     * device copy is made and uploaded at the start of a batch call, only while a trim is in force.  Configuration like the dither: in no blob. */
    std::vector<double> trim_gain;
    double *d_trim = nullptr;
    /* the delivery (gdg_batch_set_delivery; deliver.h): 1 = off (never set, or set to 1), 2 or 4: every encoded port of gdg_batch_run and
     * gdg_batch_stream_step leaves the device at a half or a quarter of the session rate.  While it is on batch_dev[BATCH_DELIVERED] holds a
     * step's decimated rows in front of the encoders and batch_dev[BATCH_DELIVER_HISTORY] the last 154 samples of every row of the window from
     * step to step; the history is zeroed by the first slice of a job and is in no checkpoint (the checkpoint calls then refuse).  Off, neither
     * exists.  Configuration like the trim: in no blob. */
    int deliver = 1;
    /* ... and the ratio behind the factor (gdg_batch_set_out_ratio): up / down, 1 / 1 = no ratio stage (never set, or set through
     * gdg_batch_set_delivery).  While one is in force deliver_tapsT holds its table as the kernel reads it, [T][up], made on the host when the
     * ratio was set; batch_dev[BATCH_DELIVER_RATIO_TABLE] its device copy, batch_dev[BATCH_DELIVER_RATIO_ROWS] a step's rows at the delivered
     * rate and batch_dev[BATCH_DELIVER_RATIO_HISTORY] the last 127 intermediate samples of every row.  Off, none of them exists. */
    int deliver_up = 1, deliver_down = 1;
    std::vector<double> deliver_tapsT;
    /* the table of the stand-alone calls' last ratio (gdg_out_ratio_rows): [T][up] on the device, made anew when another ratio is asked for */
    double *d_ratio_taps = nullptr;
    int d_ratio_up = 0, d_ratio_down = 0;
    /* the blend outputs (gdg_batch_set_blends; blend.h): weighted sums of this context's chain rows as the ports behind the metronome's; an
     * empty list = off (never set, or set with 0 blends).  While blends are in force a batch window has nch + 3 + count() rows and the device
     * copy of the table -- first | channel | delay | weight | gain, made and uploaded at the start of a batch call -- exists; off, neither does.
     * While one of the delays is not 0 (gdg_batch_set_blends_delayed) batch_dev[BATCH_BLEND_HISTORY] holds the chain rows' last 4096 samples
     * from step to step; it is zeroed by the first slice of a job and is in no checkpoint (the checkpoint calls then refuse).
     * Configuration like the trim: in no blob. */
    BlendSet blend;
    unsigned char *d_blend = nullptr;
    size_t d_blend_cap = 0;
    /* the list records (report_sections.h, LIST_KINDS; blend.h), what puts each of the five kinds in force (list_in_force): the blend fits
     * (gdg_batch_fit_enable), the Gram list (gdg_batch_gram_enable: the listed ports in list order), the tap fits (gdg_batch_tapfit_enable)
     * and the transfer list (gdg_batch_transfer_enable) as the table of ints a launch reads, empty = off; the records of the delivered rows
     * (gdg_batch_out_records_enable) as a switch: they have no list, every port of the call is recorded.  While kind k's table is in force
     * batch_dev[BATCH_FIT_TABLE + k] holds it -- uploaded at the start of a batch call; while a kind is in force a download half has room for
     * its [rows][window] elements behind the four kinds' sections and the lists' before it; off, neither exists.  While the delivered rows'
     * switch is on batch_dev[BATCH_DELIVERED_REC_HISTORY] holds the 23 samples every port keeps from step to step and
     * batch_dev[BATCH_DELIVERED_REC_SPANS] the block spans of a slice's steps, which out_rec_spans holds on the host until the slice has run;
     * off, neither exists.  Configuration like the blends: in no blob. */
    FitSet fit;
    std::vector<int> gram_port;
    TapFitSet tapfit;
    TransferSet transfer;
    bool out_rec_on = false;
    std::vector<unsigned long long> out_rec_spans;
    /* ... and their records of the last completed batch call, one store per kind: [rows][blocks] elements of `elem` bytes ([fits][blocks]
     * records, [blocks][P (P + 1) / 2], [blocks][D] and [blocks][n_pairs (4096 / D + 1) 4] doubles, [ports][blocks] records of 40 bytes)
     * beside the four kinds' and by their rule: a call that collects (`live`, decided when it begins) fills the store step by step and
     * validates it at its end; a master finish collects none.  `count`: the entries the list had when the call began (fits, ports, tap
     * fits, pairs; the call's ports). */
    struct ListRecords {
        bool live = false, valid = false;
        int count = 0;
        size_t rows = 0, elem = 0, blocks = 0;
        std::vector<unsigned char> store;
    } list_rec[LIST_KINDS];
    /* the loudness records (include/gdg.h, LOUDNESS; api_loudness.cpp): a path of its own beside the kinds above.  While the switch is on
     * (gdg_batch_loudness_enable) d_state holds the [ports][7] doubles every port keeps from step to step and d_records the [ports][hops] hop
     * sums of the running or the last slice, which come down when gdg_batch_loudness asks; off, neither exists.  `live`: the running slice
     * collects (decided when it begins); `valid`: the last one completed.  d_own: the state of a stand-alone call that was given none. */
    struct Loudness {
        bool on = false, live = false, valid = false;
        double *d_state = nullptr, *d_records = nullptr, *d_own = nullptr;
        size_t state_cap = 0, records_cap = 0, own_cap = 0;
        int ports = 0;
        size_t hops = 0;
        unsigned long long hop_base = 0;
        uint32_t rate = 0;
        gdg_loudness_params par;
    } loud;
    /* ... and the spans of the stand-alone calls' last launch (gdg_block_out_rows): the host's copy, which the upload reads, and the device's */
    std::vector<unsigned long long> out_rows_spans;
    unsigned long long *d_out_rows_spans = nullptr;
    size_t d_out_rows_spans_cap = 0;
    /* options "stat_batch_upload_bytes" / "stat_batch_resampled_samples": input file bytes moved to the device and output samples the
     * Lanczos sum was evaluated for, by the last batch run call or slice; the int fields are made (saturated) when they are read */
    unsigned long long batch_up_bytes = 0, batch_resampled = 0;
    int stat_batch_up_bytes = 0, stat_batch_resampled = 0;
    /* the master mix of a job or a slice (finish_master): the partials of a piece gathered into a pinned slab half, the encoded piece back through another */
    PinnedHalves h_fin_up, h_fin_down;
    hipEvent_t fin_up[2] = { nullptr, nullptr }, fin_down[2] = { nullptr, nullptr };     /* a half's upload has left it / its download has landed */
    /* channel groups of the host-buffer paths: group g's upload, kernels and download run on stream g, so one group's
     * PCIe transfers overlap the other groups' kernels (channels are independent) */
    int plan_groups = 1;
    std::vector<size_t> plan_bounds;           /* first active index of every channel group (+ the end) the plan was built for */
    int overlap_groups = 0;                    /* 0: automatic (device_groups) */
    bool groups_pending = false;               /* group streams hold work the context's stream has not been ordered after */
    std::vector<hipStream_t> gstreams;
    std::vector<hipEvent_t> gjoin;
    hipEvent_t gfork = nullptr;
    CopyPool *copy_pool = nullptr;             /* host copy workers of the host-buffer paths, made on first use */
    CopyPool *copy_pool_up = nullptr;          /* ... a second set for the batch run's upload side: the next step's bytes are gathered while this step's are scattered */
    /* metronome (metronome/metronome.go): sounds in HBM, the two counters on the host */
    double *d_tick = nullptr, *d_tock = nullptr;
    uint32_t n_tick = 0, n_tock = 0;
    uint32_t met_sample_counter = 0, met_tick_counter = 0, met_beats = 4, met_bpm = 120, met_sr = 96000;
};

/* a delivery other than the session rate is in force: a factor, a ratio behind it, or both */
static inline bool delivery_on(const gdg_ctx *ctx) { return ctx->deliver > 1 || gdg_deliver_ratio_on(ctx->deliver_up, ctx->deliver_down); }

inline int fail(const gdg_ctx *ctx, int code, const char *fmt, ...) {       /* one definition, one mutex, for all files */
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) {
        static std::mutex mu;                      /* the batch run's helper thread may fail beside the calling thread (api_batch.cpp) */
        std::lock_guard<std::mutex> lk(mu);
        ctx->err = buf;
    }
    return code;
}

/* what a call without a context refuses (gdg_trim_from_true_peak): kept per thread, read by gdg_last_error(NULL) */
inline std::string &free_error() { static thread_local std::string e; return e; }
inline void set_free_error(const char *msg) { free_error() = msg; }

/* Device-resident calls may leave their channel groups running on streams of their own (process_rows, `free_run`); whatever
 * touches the context next -- any entry point -- first makes the context's stream wait for them. */
static inline void join_groups(gdg_ctx *ctx) {
    if (!ctx->groups_pending) return;
    for (size_t g = 0; g < ctx->gstreams.size() && g < ctx->gjoin.size(); g++) {
        hipEventRecord(ctx->gjoin[g], ctx->gstreams[g]);
        hipStreamWaitEvent(ctx->stream, ctx->gjoin[g], 0);
    }
    ctx->groups_pending = false;
}
/* the context's stream behind the premac launch; `keep` = the caller changes no state (synchronize, stream, profiling): the sums stay usable */
static inline void join_premac(gdg_ctx *ctx, bool keep) {
    if (ctx->premac_outstanding) {
        hipStreamWaitEvent(ctx->stream, ctx->ev_premac, 0);
        ctx->premac_outstanding = false;
    }
    if (!keep) ctx->premac_valid = false;
}
/* the sums made ahead of the next frames (Shape FUSED_AHEAD) are never read again: a new epoch */
static inline void drop_fir_ahead(gdg_ctx *ctx) {
    ctx->fir_ahead_epoch = ctx->fir_ahead_epoch == 0xffffffffu ? 1u : ctx->fir_ahead_epoch + 1u;
    ctx->fir_ahead_calls = 0;
}
static inline void stat_add(int &counter) { if (counter < 0x7fffffff) counter++; }
/* `keep_fir_sums`: the call changes nothing the sums made ahead of the next frames read -- filters, delay lines, frame counters, ring
 * layout, plan (caller data, codecs, tuner, spatializer, meters, the host-buffer process calls, whose plan process_rows checks itself) */
static inline void enter(gdg_ctx *ctx, bool read_only = false, bool keep_fir_sums = false) {
    hipSetDevice(ctx->device);
    join_groups(ctx);
    join_premac(ctx, read_only);
    if (!read_only && !keep_fir_sums) drop_fir_ahead(ctx);
}
static inline void enter_keep_fir_sums(gdg_ctx *ctx) { enter(ctx, false, true); }

/* the parameter index of an overdrive's / distortion's / excess's oversampling (0 none, 1 "2", 2 "4"); -1: the unit type has none */
static inline int shaper_os_param(int type) {
    return type == GDG_UNIT_OVERDRIVE ? 5 : type == GDG_UNIT_DISTORTION ? 3 : type == GDG_UNIT_EXCESS ? 2 : -1;
}

#define HIP_TRY(ctx, call)                                                                          \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess) return fail(ctx, GDG_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

static inline double decibels_to_factor(int32_t decibels) {          /* effects/effects.go:389-394 */
    double e = 0.05 * (double)decibels;
    return pow(10.0, e);
}

static inline double lanczos_kernel(double x, double a) {             /* resample/resample.go:10-31 */
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


/* ---- shared between the source files ------------------------------------------------------------------------------------------- */
/* what a host-buffer entry point does around group g's kernels, on group g's stream (upload before, download after) */
typedef std::function<hipError_t(int g, hipStream_t s)> GroupHook;

hipEvent_t take_event(gdg_ctx *ctx);
struct ProfScope {
    gdg_ctx *ctx; int kind; hipStream_t st; hipEvent_t a = nullptr, b = nullptr; bool on = false, attached = false;
    ProfScope(gdg_ctx *c, int k, hipStream_t s = nullptr, bool attach = false) : ctx(c), kind(k), st(s ? s : c->stream), attached(attach) {
        on = ctx->prof_now && ((ctx->profiling & 1u) || (ctx->profiling & (1u << (k + 1))));
        if (on) { a = take_event(ctx); b = take_event(ctx); if (!attached) hipEventRecord(a, st); }
    }
    ~ProfScope() {
        if (on) { if (!attached) hipEventRecord(b, st); ctx->prof.push_back(ProfEvent{ kind, a, b }); }
    }
};

void numa_bind_thread(const std::vector<int> &cpus);

/* Host copy workers.  One core moves pageable memory at ~10 GB/s, which made the 2 x 32 MiB of a 512-channel block cost 3 ms -- more
 * than the whole chain -- so staging copies are spread over a few threads (env GDG_COPY_THREADS, default 8).  The workers are
 * PERSISTENT: created on a context's first host-buffer call and parked on a condition variable between jobs (spawning and joining
 * std::threads on every call cost 60-100 us per call, twice per block).  One pool PER CONTEXT since round 4: with one process-wide
 * pool only one of G shards copying at the same time got the workers and the others copied on their caller's thread alone
 * (the reference's deployment is G shards in one process, controller.go:3262-3269).  Joined and freed with the context.
 * fork(): a child inherits the pool object but none of its threads; it finds another pid in the pool and copies inline. */
class CopyPool {
public:
    /* cpus: the workers' CPUs (the device's NUMA node), empty = wherever the scheduler puts them */
    explicit CopyPool(int workers, std::vector<int> cpus = {}) : cpus_(std::move(cpus)), pid_(getpid()) {
        for (int i = 0; i < workers; i++) threads_.emplace_back([this, i]() { numa_bind_thread(cpus_); loop((size_t)i + 1); });
    }
    ~CopyPool() {                               /* only in the process that made the pool (destroy_copy_pool) */
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true; gen_++;
        }
        cv_work_.notify_all();
        for (auto &t : threads_) t.join();
    }
    size_t slots() const { return threads_.size() + 1; }
    bool usable() const { return pid_ == getpid(); }
    /* slice t of T runs fn(t); the caller takes slice 0 and returns when all slices are done */
    void run(size_t T, const std::function<void(size_t)> &fn) {
        if (T <= 1) { fn(0); return; }
        std::unique_lock<std::mutex> job(job_mu_, std::try_to_lock);
        if (!job.owns_lock()) { for (size_t t = 0; t < T; t++) fn(t); return; }
        {
            std::lock_guard<std::mutex> lk(mu_);
            fn_ = &fn; T_ = T; pending_ = T - 1; gen_++;
        }
        cv_work_.notify_all();
        fn(0);
        std::unique_lock<std::mutex> lk(mu_);
        cv_done_.wait(lk, [this]() { return pending_ == 0; });
        fn_ = nullptr;
    }
private:
    void loop(size_t slot) {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(size_t)> *fn = nullptr;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_work_.wait(lk, [&]() { return gen_ != seen; });
                if (stop_) return;
                seen = gen_;
                if (slot < T_) fn = fn_;
            }
            if (!fn) continue;
            (*fn)(slot);
            std::lock_guard<std::mutex> lk(mu_);
            if (--pending_ == 0) cv_done_.notify_one();
        }
    }
    std::vector<std::thread> threads_;
    std::mutex job_mu_, mu_;
    std::condition_variable cv_work_, cv_done_;
    const std::function<void(size_t)> *fn_ = nullptr;
    size_t T_ = 0, pending_ = 0;
    uint64_t gen_ = 0;
    bool stop_ = false;
    std::vector<int> cpus_;
    pid_t pid_;
};

Unit *get_unit(gdg_ctx *ctx, int handle);
bool segf_unit_ok(const Unit &u, int frames, uint32_t sample_rate);
bool reverb_ahead_ok(int frames, uint32_t sample_rate);
hipError_t pinned_alloc(gdg_ctx *ctx, void **p, size_t bytes);
inline void PinnedHalves::release() {
    for (int h = 0; h < 2; h++) {
        if (half[h]) hipHostFree(half[h]);
        half[h] = nullptr;
    }
    cap = 0;
}
inline hipError_t PinnedHalves::grow(gdg_ctx *ctx, size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    release();
    for (int h = 0; h < 2; h++) {
        const hipError_t e = pinned_alloc(ctx, (void **)&half[h], bytes);
        if (e != hipSuccess) return e;
    }
    cap = bytes;
    return hipSuccess;
}
int build_plan(gdg_ctx *ctx, const std::vector<int> &active, const double *d_in, double *d_out, int frames, uint32_t sample_rate,
                      int stride, int stride_out, bool rows_by_channel, int G, const std::vector<size_t> &bounds);
int check_device_error(gdg_ctx *ctx);
int ensure_io(gdg_ctx *ctx, int which, size_t bytes);
int ensure_staging(gdg_ctx *ctx);
int fir_tables(gdg_ctx *ctx, int P, double2 **tw, double2 **tw2);
/* the band spectrum's tables: the window weights (made and uploaded with the first use) and the 4096-point transform's twiddles */
int spectrum_tables(gdg_ctx *ctx, const double **win, double2 **tw, double2 **tw2);
/* api_io.cpp: the true-peak record's 3 x 24 taps, built on the host with the first use (true_peak_taps.h) */
const gdg_true_peak_table &true_peak_table();
/* api_io.cpp: the ratio stage's table (include/gdg.h, DELIVERY), float64 on the host: [up][T] as gdg_out_ratio_taps hands it out, or [T][up] as the kernel reads it; returns T (0: no table) */
int deliver_ratio_table(int up, int down, bool transposed, std::vector<double> &taps);
/* ... and what every call refuses of a ratio, worded once: GDG_OK, or GDG_ERR_INVALID with the ratio (and, unreduced, the reduced pair) named */
int deliver_ratio_check(gdg_ctx *ctx, const char *what, int up, int down);
int fir_transform_size(int frames);
int meter_rows(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int port0, int n_ports, int frames, uint32_t sample_rate);
int numa_rebind(gdg_ctx *ctx, int mode);
int numa_target(const gdg_ctx *ctx, const std::vector<int> **cpus);
int prepare_unit(gdg_ctx *ctx, Unit &u, int frames, uint32_t sample_rate, gdg_seg_unit &d, int chk = GDG_CHK);
int prepare_fir(gdg_ctx *ctx, Unit &u, int hop, uint32_t sample_rate);
int process_rows(gdg_ctx *ctx, const std::vector<int> &active, const double *d_in, double *d_out, int frames, uint32_t sample_rate,
                        int stride = 0, bool rows_by_channel = false, int groups = 1, const GroupHook *before = nullptr, const GroupHook *after = nullptr,
                        int window = 1, int stride_out = 0, const std::vector<size_t> *group_bounds_in = nullptr);
int ensure_spatializer(gdg_ctx *ctx);
int spatialize_rows(gdg_ctx *ctx, const double *d_in, int in_stride, double *d_left, int out_stride, int frames);
int tuner_enqueue_rows(gdg_ctx *ctx, const double *d_samples, size_t stride, int frames, uint32_t sample_rate);
void copy_rows_parallel(gdg_ctx *ctx, size_t a, size_t b, const std::function<void(size_t)> &copy_row, size_t row_bytes, int which = 0);      /* which: 1 = the upload side's workers */
void destroy_copy_pool(CopyPool *p);
void ensure_copy_pool(gdg_ctx *ctx, int which);     /* makes the pool NOW, on the calling thread (option "numa" = 2 binds the workers to the node of the thread that makes them) */

/* ---- state blobs and checkpoints (api_state.cpp, api_checkpoint.cpp; the copies: state.hip) --------------------------------------- */
static inline size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }

/* The pieces of one launch, the prefix table of their chunks, and the launch (synchronous: the caller's buffers are complete after it) */
struct Pieces {
    std::vector<gdg_state_piece> p;
    void add(const void *src, void *dst, size_t bytes) { if (bytes) p.push_back(gdg_state_piece{ src, dst, (unsigned long long)bytes }); }
    /* a region of `bytes` and the zeros that round it up to 16 in the blob */
    void add_padded(const void *src, void *dst, size_t bytes, bool dst_is_blob) {
        add(src, dst, bytes);
        const size_t pad = round16(bytes) - bytes;
        if (pad && dst_is_blob) add(nullptr, (char *)dst + bytes, pad);
    }
    void append(const Pieces *more) { if (more) p.insert(p.end(), more->p.begin(), more->p.end()); }
    int run(gdg_ctx *ctx) {
        if (p.empty()) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); return GDG_OK; }
        std::vector<unsigned> first(p.size());
        unsigned long long chunks = 0;
        for (size_t i = 0; i < p.size(); i++) {
            first[i] = (unsigned)chunks;
            chunks += (p[i].bytes + GDG_STATE_CHUNK - 1) / GDG_STATE_CHUNK;
        }
        if (chunks > 0x7fffffffull) return fail(ctx, GDG_ERR_INVALID, "state: %llu chunks in one launch", chunks);
        const size_t pb = round16(p.size() * sizeof(gdg_state_piece));
        void *d = nullptr;
        HIP_TRY(ctx, ctx->arena.alloc(&d, pb + first.size() * sizeof(unsigned)));
        std::vector<unsigned char> host(pb + first.size() * sizeof(unsigned), 0);
        memcpy(host.data(), p.data(), p.size() * sizeof(gdg_state_piece));
        memcpy(host.data() + pb, first.data(), first.size() * sizeof(unsigned));
        hipError_t e = hipMemcpyAsync(d, host.data(), host.size(), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess)
            e = gdg_launch_state_copy((const gdg_state_piece *)d, (const unsigned *)((char *)d + pb), (int)p.size(), (unsigned)chunks, ctx->stream);
        hipError_t w = hipStreamSynchronize(ctx->stream);
        ctx->arena.release(d);
        if (e != hipSuccess) return fail(ctx, GDG_ERR_HIP, "state copy: %s", hipGetErrorString(e));
        if (w != hipSuccess) return fail(ctx, GDG_ERR_HIP, "state copy: %s", hipGetErrorString(w));
        return GDG_OK;
    }
};

/* api_state.cpp, for a checkpoint: every channel's state into / out of a 16-byte-aligned device buffer, the caller's own pieces (`extra`)
 * riding in the same launch as the state's.  state_check_device only reads: header, structure and every layout key against the layouts
 * a load WOULD build (what gdg_state_load checks before it touches the target). */
int state_save_device_with(gdg_ctx *ctx, void *d_blob, size_t capacity, const Pieces *extra);
int state_check_device(gdg_ctx *ctx, const void *d_blob, size_t bytes);
int state_load_device_with(gdg_ctx *ctx, const void *d_blob, size_t bytes, const Pieces *extra);
/* api_batch.cpp: the job a run describes (validated, nothing of the context touched); the context's BATCH_CARRY buffer */
int stream_job(gdg_ctx *ctx, const gdg_batch_input *inputs, int n_inputs, const gdg_batch_options *opt, bool shard, size_t job_samples,
               bool run_metronome, gdg_ctx::BatchStreamState &job, bool meters_at_open = true);
int batch_carry_buffer(gdg_ctx *ctx, double **d_carry);
/* api_batch.cpp: what a shard's entry point `what` refuses while list records are in force -- fits, then the Gram list, then tap fits, then transfer pairs; GDG_OK: none is (or no context) */
int lists_refused(gdg_ctx *ctx, const char *what);
/* api_loudness.cpp: what the entry point `what` refuses while the loudness records are on, `why` in a few words; GDG_OK: they are off (or no context) */
int loudness_refused(gdg_ctx *ctx, const char *what, const char *why);
/* api_loudness.cpp, for the slice runner: a slice of `samples` samples at the job's sample `pos` begins (its buffers, zeroed by a job's first
 * slice); a step's rows, the job's samples [first, first + count), are measured; the slice has ended with rc.  Off: nothing is done */
int loudness_slice_begin(gdg_ctx *ctx, int ports, size_t pos, size_t samples, uint32_t rate);
int loudness_step(gdg_ctx *ctx, const double *d_rows, size_t row_stride, size_t first, size_t count);
int loudness_slice_end(gdg_ctx *ctx, int rc);
/* ... its device buffers go (the caller has waited for whatever reads them); the bytes they hold */
void loudness_release(gdg_ctx *ctx);
size_t loudness_device_bytes(const gdg_ctx *ctx);
/* loudness.hip */
hipError_t gdg_launch_block_loudness(const double *d_rows, size_t row_stride, unsigned n_rows, unsigned long long first, unsigned long long count, uint32_t rate,
                                     unsigned long long hop_base, unsigned long long hops_room, const gdg_loudness_params &par, double *d_state, double *d_records, hipStream_t s);
/* api_io.cpp: a list of fits against gdg_fit_check (blend.h), refused in the words of `what`; n_rows < 0: the port count is not known yet */
int fit_list_check(gdg_ctx *ctx, const char *what, int n_fits, const int *first, const int *port, const int *target, int n_rows);
/* api_io.cpp: a Gram list of `least` to GDG_GRAM_MAX_PORTS ports against blend.h's checks, refused in the words of `what`; n_rows < 0: the port count is not known yet */
int gram_list_check(gdg_ctx *ctx, const char *what, const int *port, int n_ports, int least, int n_rows);
/* api_io.cpp: a list of tap fits against gdg_tapfit_check (blend.h), refused in the words of `what`; n_rows < 0: the port count is not known yet */
int tapfit_list_check(gdg_ctx *ctx, const char *what, int n_fits, const int *first, const int *port, const int *target, const int *taps, int n_rows);
/* api_io.cpp: a transfer list against gdg_transfer_check (blend.h), refused in the words of `what`; n_rows < 0: the port count is not known yet */
int transfer_list_check(gdg_ctx *ctx, const char *what, int n_pairs, const int *port, const int *target, int group, int n_rows);
/* the map in force has a reader: what a checkpoint cannot record yet */
static inline bool batch_sources_shared(const gdg_ctx *ctx) { return sources_have_reader(ctx->batch_source); }
/* a batch call begins: every kind's records of the call before are gone; a kind that is switched on gets zeroed records for `ports` x
 * `blocks`.  `align`: this call may collect alignment records (the finish calls never do) */
static inline void report_begin(gdg_ctx *ctx, int ports, size_t blocks, bool align = true, int blend_ports = 0) {
    ctx->spec_live_edges = ctx->spec_edges;
    ctx->align_live_ref.clear();
    for (gdg_ctx::ListRecords &R : ctx->list_rec) R.valid = R.live = false;      /* a call that collects list records says so itself (list_begin) */
    ctx->loud.valid = ctx->loud.live = false;                                    /* ... and so does one that collects loudness records (loudness_slice_begin) */
    /* any other count was refused when the job was described; a list without the call's blend ports: each of them references itself */
    if (align && ((int)ctx->align_ref.size() == ports || (blend_ports > 0 && (int)ctx->align_ref.size() == ports - blend_ports))) {
        ctx->align_live_ref = ctx->align_ref;
        for (int p = (int)ctx->align_ref.size(); p < ports; p++) ctx->align_live_ref.push_back(p);
        ctx->align_live_lag = ctx->align_lag;
    }
    const bool on[REPORT_KINDS] = { ctx->report_on, !ctx->spec_live_edges.empty(), !ctx->align_live_ref.empty(), ctx->tp_on };
    const size_t n_bands = ctx->spec_live_edges.empty() ? 0 : ctx->spec_live_edges.size() - 1;      /* the bands a call collects are its live edges' */
    for (int k = 0; k < REPORT_KINDS; k++) {
        gdg_ctx::ReportKind &K = ctx->report[k];
        K.valid = false;
        K.live = on[k];
        if (!K.live) continue;
        K.ports = ports;
        K.blocks = blocks;
        K.elem = report_elem(k, n_bands);
        K.store.assign((size_t)ports * blocks * K.elem, 0);
    }
}
/* kind k in force for a call of `ports` ports: the table of ints a launch reads (the fits', tap fits' and transfer list's tables, the Gram
 * list's ports; the delivered rows' records have none), the entries it counts (fits, ports, tap fits, pairs; the call's ports) and what it
 * sends down per block; nothing in force: no int, count 0, a shape that is off */
struct ListInForce { const int *table; size_t ints; int count; ListShape shape; };
static inline ListInForce list_in_force(const gdg_ctx *ctx, int k, int ports) {
    if (k == LIST_FIT) return { ctx->fit.table.data(), ctx->fit.table.size(), ctx->fit.count(), { (size_t)ctx->fit.count(), ctx->fit.count() ? (size_t)FIT_RECORD_BYTES : 0 } };
    if (k == LIST_GRAM) return { ctx->gram_port.data(), ctx->gram_port.size(), (int)ctx->gram_port.size(), { 1, gram_record_bytes(ctx->gram_port.size()) } };
    if (k == LIST_TAPFIT) return { ctx->tapfit.table.data(), ctx->tapfit.table.size(), ctx->tapfit.count(), { 1, ctx->tapfit.doubles() * sizeof(double) } };
    if (k == LIST_TRANSFER) return { ctx->transfer.table.data(), ctx->transfer.table.size(), ctx->transfer.count(), { 1, ctx->transfer.doubles() * sizeof(double) } };
    if (!ctx->out_rec_on) return { nullptr, 0, 0, { 0, 0 } };
    return { nullptr, 0, ports, { (size_t)ports, (size_t)DELIVERED_RECORD_BYTES } };
}
/* the first three kinds' launchers take one argument list (gdg_internal.h): rows, stride, n_rows, samples, block, host table, device table,
 * count, records, stream; the transfer records' takes its transform's table, the delivered rows' records' their spans and history */
typedef hipError_t ListLaunch(const double *, size_t, unsigned, size_t, unsigned, const int *, const int *, unsigned, void *, hipStream_t);
enum { LIST_LAUNCHERS = 3 };
static ListLaunch *const list_launch[LIST_LAUNCHERS] = { gdg_launch_block_fit, gdg_launch_block_gram, gdg_launch_block_tapfit };
static_assert(LIST_FIT == 0 && LIST_GRAM == 1 && LIST_TAPFIT == 2 && LIST_TRANSFER == LIST_LAUNCHERS, "list_launch[k] is kind k's launcher for the kinds in front of LIST_TRANSFER only");
/* behind report_begin, by the calls that collect list records: zeroed records for kind k in force x `blocks` */
static inline void list_begin(gdg_ctx *ctx, int k, size_t blocks, int ports) {
    const ListInForce L = list_in_force(ctx, k, ports);
    gdg_ctx::ListRecords &R = ctx->list_rec[k];
    R.live = L.shape.on();
    if (!R.live) return;
    R.count = L.count;
    R.rows = L.shape.rows;
    R.elem = L.shape.elem;
    R.blocks = blocks;
    R.store.assign(R.rows * blocks * R.elem, 0);
}
/* a step's section of kind k ([rows][w] elements) that has come down, into the store under the blocks from b0 on */
static inline void list_file(gdg_ctx *ctx, int k, const unsigned char *section, size_t w, size_t b0) {
    gdg_ctx::ListRecords &R = ctx->list_rec[k];
    list_file_rows(R.store.data(), R.blocks, { R.rows, R.elem }, section, w, b0);
}
/* ... and has completed (rc == GDG_OK) or not */
static inline int report_end(gdg_ctx *ctx, int rc) {
    for (gdg_ctx::ListRecords &R : ctx->list_rec) {
        R.valid = R.live && rc == GDG_OK;
        R.live = false;
    }
    for (gdg_ctx::ReportKind &K : ctx->report) {
        K.valid = K.live && rc == GDG_OK;
        K.live = false;
    }
    ctx->spec_live_edges.clear();
    ctx->align_live_ref.clear();
    return rc;
}
/* the kinds the running call collects, with their element sizes */
static inline ReportLive report_live(const gdg_ctx *ctx) {
    ReportLive live;
    for (int k = 0; k < REPORT_KINDS; k++) live.elem[k] = ctx->report[k].live ? ctx->report[k].elem : 0;
    return live;
}
/* rows `rows` of a section that has come down ([..][w] elements of kind k) into the kind's store, under the blocks from b0 on */
static inline void report_file(gdg_ctx *ctx, int k, const unsigned char *section, const std::vector<size_t> &rows, size_t w, size_t b0) {
    gdg_ctx::ReportKind &K = ctx->report[k];
    for (size_t o : rows) memcpy(&K.store[(o * K.blocks + b0) * K.elem], section + o * w * K.elem, w * K.elem);
}
#define GDG_STREAM_CARRY 8            /* source frames kept per resampled input: the window reaches 2 back and 3 ahead, so a step looks at most 6 back */
/* gdg_ctx::batch_dev, slot by slot (the slice runner, api_batch.cpp) */
enum {
    BATCH_INPUTS,                          /* [N][slice] decoded (and resampled) inputs */
    BATCH_WINDOW,                          /* [N + 3 + blends][window] one step's outputs, the blend rows (gdg_batch_set_blends) behind the metronome's */
    BATCH_ENCODED,                         /* two halves of a step on its way down: encoded rows, a shard's float64 rows */
    BATCH_CARRY,                           /* [N][GDG_STREAM_CARRY] source frames every resampled input keeps for its next step */
    BATCH_UPLOAD,                          /* two halves of a step on its way up: descriptors, then the inputs' bytes */
    BATCH_SOURCE,                          /* two halves of the resampler's source frames: [kept | this step's] per resampled input */
    BATCH_BLEND_HISTORY,                   /* [N][GDG_BLEND_MAX_DELAY] the chain rows' last samples of the step before, only while a blend delay is in force */
    BATCH_FIT_TABLE,                       /* [fits][target | terms | port[8]] the blend fits' table, only while fits are in force (gdg_batch_fit_enable) */
    BATCH_GRAM_PORTS,                      /* [P] the Gram list's ports, only while a list is in force (gdg_batch_gram_enable) */
    BATCH_TAPFIT_TABLE,                    /* [fits][target | terms | taps | port[4] | offset | tile] the tap fits' table, only while tap fits are in force (gdg_batch_tapfit_enable) */
    BATCH_TRANSFER_TABLE,                  /* [pairs][port | target], then the group width: the transfer list's table, only while one is in force (gdg_batch_transfer_enable) */
    BATCH_DELIVERED,                       /* [N + 3 + blends][window / R] one step's rows at the delivered rate, what the encoders read; only while a delivery factor is in force (gdg_batch_set_delivery) */
    BATCH_DELIVER_HISTORY,                 /* [N + 3 + blends][154] the window rows' last samples of the step before, only while a delivery factor is in force */
    BATCH_DELIVER_RATIO_ROWS,              /* [N + 3 + blends][pitch] one step's rows behind the ratio stage, what the encoders then read; only while a delivery ratio is in force (gdg_batch_set_out_ratio) */
    BATCH_DELIVER_RATIO_HISTORY,           /* [N + 3 + blends][127] the intermediate rows' last samples of the step before, only while a delivery ratio is in force */
    BATCH_DELIVER_RATIO_TABLE,             /* [T][up] the ratio's taps, only while a delivery ratio is in force */
    BATCH_DELIVERED_REC_HISTORY,           /* [N + 3 + blends][23] the encoders' rows' last samples of the step before, only while the delivered rows' records are on (gdg_batch_out_records_enable) */
    BATCH_DELIVERED_REC_SPANS,             /* per step of a slice its w + 1 block spans, 64-bit, only while the delivered rows' records are on */
    BATCH_DEV_SLOTS
};
static_assert(sizeof(gdg_ctx::batch_dev) / sizeof(void *) == BATCH_DEV_SLOTS && sizeof(gdg_ctx::batch_dev_cap) / sizeof(size_t) == BATCH_DEV_SLOTS,
              "gdg_ctx::batch_dev and batch_dev_cap have one entry per slot");
static_assert(BATCH_GRAM_PORTS == BATCH_FIT_TABLE + LIST_GRAM && BATCH_TAPFIT_TABLE == BATCH_FIT_TABLE + LIST_TAPFIT && BATCH_TRANSFER_TABLE == BATCH_FIT_TABLE + LIST_TRANSFER,
              "BATCH_FIT_TABLE + k is list kind k's slot");
int ensure_tuner(gdg_ctx *ctx);

#pragma GCC visibility pop

#endif
