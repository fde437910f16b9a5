/*
 * gdg_host.hpp -- host-side mirror of the reference's Go interfaces for the hot path, written in
 * C++ because the build image has no Go toolchain (the Go shim a maintainer would compile is in
 * ../go/ and INTEGRATION.md; it has the same structure as this file).
 *
 *   effects::Unit       <->  effects.Unit       (effects/effects.go:83-91)     7 methods
 *   effects::Parameter  <->  effects.Parameter  (effects/effects.go:69-78)
 *   signal::Chain       <->  signal.Chain       (signal/signal.go:21-36)       14 methods
 *   filter::Filter / ImpulseResponses  <->  filter.Filter / filter.ImpulseResponses (filter/filter.go:64-95)
 *
 * Same names, argument meaning and error strings.  Go's `error` is a std::string here (empty =
 * nil).  Parameter tables, name lookup, range checks and the power-amp filter compile
 * (Reduce / Normalize / Multiply / Add, effects/poweramp.go:25-127) live here; only resolved
 * integers, taps and sample buffers cross the C-ABI of include/gdg.h.  All audio is computed by
 * libgdg.so on the GPU: nothing in this file processes samples.
 */
#ifndef GDG_HOST_HPP
#define GDG_HOST_HPP

#include <condition_variable>
#include <cstdint>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/gdg.h"      /* the C-ABI the twin is written against (gdg_ctx, gdg_batch_input, gdg_batch_options ...) */
#include "batch_records.h"          /* the nine kinds of records a batch call keeps: one table, one store per kind */

#define GDG_HOST_MAX_FRAMES 8192      /* controller/controller.go:36 BLOCK_SIZE */

namespace gdg {

using Error = std::string;          /* "" == nil */

namespace filter {

class Filter {
public:
    Filter(std::vector<double> coeffs, uint32_t sampleRate, double gainCompensation, std::string name);
    std::pair<std::shared_ptr<Filter>, Error> Add(const std::shared_ptr<Filter> &other) const;   /* filter.go:167-253 */
    std::vector<double> Coefficients() const;                                                     /* :258-265 */
    std::shared_ptr<Filter> Multiply(double scalar) const;                                        /* :270-323 */
    std::shared_ptr<Filter> Normalize() const;                                                    /* :328-336 */
    std::shared_ptr<Filter> Reduce(uint32_t order) const;                                         /* :520-604 */
    uint32_t SampleRate() const { return sampleRate_; }                                           /* :609-613 */
    const std::string &Name() const { return name_; }
private:
    std::vector<double> data_;
    uint32_t sampleRate_;
    double gainCompensation_;
    std::string name_;
};

std::shared_ptr<Filter> Empty(uint32_t sampleRate);                                               /* :807-845 */
std::shared_ptr<Filter> FromCoefficients(const std::vector<double> &coeffs, uint32_t sampleRate, const std::string &name);  /* :850-890 */
std::vector<uint32_t> SampleRates();                                                              /* :895-900 */

/* filter.ImpulseResponses (filter.go:64-67).  The reference fills it from ir/index.json + WAV files
 * (filter.Import, host I/O, out of scope); here entries are added from memory. */
class ImpulseResponses {
public:
    void Add(const std::string &name, uint32_t sampleRate, int32_t compensationDecibels, const std::vector<double> &taps);
    std::shared_ptr<Filter> CreateFilter(const std::string &name, uint32_t sampleRate) const;    /* :619-658 */
    std::vector<std::string> Names() const;                                                       /* :663-699 */
private:
    struct Entry { std::string name; uint32_t sampleRate; double gainCompensation; std::vector<double> data; };
    std::vector<Entry> responses_;
};

}  // namespace filter

namespace effects {

enum { PARAMETER_TYPE_INVALID = 0, PARAMETER_TYPE_DISCRETE, PARAMETER_TYPE_NUMERIC };   /* effects.go:11-15 */
enum {                                                                                     /* effects.go:21-43 */
    UNIT_SIGNALGENERATOR = 0, UNIT_NOISEGATE, UNIT_BANDPASS, UNIT_AUTOWAH, UNIT_AUTOYOY, UNIT_COMPRESSOR, UNIT_OCTAVER,
    UNIT_EXCESS, UNIT_FUZZ, UNIT_OVERDRIVE, UNIT_DISTORTION, UNIT_TONESTACK, UNIT_CHORUS, UNIT_FLANGER, UNIT_PHASER,
    UNIT_TREMOLO, UNIT_RINGMODULATOR, UNIT_DELAY, UNIT_REVERB, UNIT_POWERAMP, UNIT_CABINET, UNIT_COUNT
};
constexpr int NUM_FILTERS = 8;                 /* effects.go:62 */
extern const char *const STRING_NONE;          /* "- NONE -" */

struct Parameter {                             /* effects.go:69-78 */
    std::string Name;
    int32_t Type = PARAMETER_TYPE_INVALID;
    std::string PhysicalUnit;
    int32_t Minimum = -1, Maximum = -1, NumericValue = -1;
    int DiscreteValueIndex = -1;
    std::vector<std::string> DiscreteValues;
};

class Unit {                                   /* effects.go:83-91 + unitStruct :96-100 */
public:
    explicit Unit(int unitType);
    ~Unit();
    std::vector<Parameter> Parameters() const;
    /* Stand-alone Process of a unit that is not in a chain: runs it as a one-slot chain on a private
     * one-channel context (device 0).  Units owned by a Chain are processed through Chain::Process. */
    void Process(const double *in, double *out, size_t n, uint32_t sampleRate);
    int Type() const { return unitType_; }
    Error SetDiscreteValue(const std::string &name, const std::string &value);
    std::pair<std::string, Error> GetDiscreteValue(const std::string &name) const;
    Error SetNumericValue(const std::string &name, int32_t value);
    std::pair<int32_t, Error> GetNumericValue(const std::string &name) const;

    /* ---- plumbing used by signal::Chain / Engine (not part of the mirrored interface) ---- */
    struct Backing { gdg_ctx *ctx = nullptr; int handle = -1; bool owns_ctx = false; };
    Backing backing;
    uint64_t paramVersion = 1, pushedParamVersion = 0;     /* resolved-integer parameters */
    uint64_t firVersion = 0, pushedFirVersion = 0;         /* power amp: current composite filter */
    std::vector<double> firTaps;                           /* taps of currentFilter (empty: zeros out) */
    uint32_t sampleRate = 0;                               /* power amp: poweramp.sampleRate */
    const filter::ImpulseResponses *impulseResponses = nullptr;
    void resolved(int32_t out[8]) const;                   /* numeric values / discrete indices of the first <= 8 parameters */
    void onSampleRate(uint32_t sampleRate);                /* poweramp.go:191-203 */
    /* Everything sync() sends to the device, taken under the unit's lock in ONE step: control-plane setters run concurrently with
     * the batch leader (controller.go:3493-3498), so versions, resolved values and taps must belong together. */
    struct Snapshot { uint64_t paramVersion, firVersion; int32_t values[8]; int nValues; std::vector<double> taps; bool withTaps; };
    Snapshot snapshot(uint64_t pushedFir) const;
private:
    friend Error PreparePowerAmp(Unit &unit, const filter::ImpulseResponses *responses);
    Error setDiscrete(const std::string &name, const std::string &value);
    Error setNumeric(const std::string &name, int32_t value);
    std::pair<std::shared_ptr<filter::Filter>, Error> compile(uint32_t sampleRate) const;   /* poweramp.go:25-127 */
    void recompile();
    int unitType_;
    mutable std::mutex mutex_;
    std::vector<Parameter> params_;
};

std::shared_ptr<Unit> CreateUnit(int unitType);                                            /* effects.go:443-516 */
Error PreparePowerAmp(Unit &unit, const filter::ImpulseResponses *responses);               /* poweramp.go:221-289 */
std::vector<std::string> ParameterTypes();                                                  /* effects.go:521-533 */
std::vector<std::string> UnitTypes();                                                       /* effects.go:538-568 */

}  // namespace effects

class Engine;

namespace signal {

class Chain {                                  /* signal.go:21-36 */
public:
    std::pair<int, Error> AppendUnit(int unitType);
    Error RemoveUnit(int id);
    Error MoveUp(int id);
    Error MoveDown(int id);
    std::pair<int, Error> UnitType(int id) const;
    Error SetBypass(int id, bool bypass);
    std::pair<bool, Error> GetBypass(int id) const;
    Error SetDiscreteValue(int id, const std::string &name, const std::string &value);
    std::pair<std::string, Error> GetDiscreteValue(int id, const std::string &name) const;
    Error SetNumericValue(int id, const std::string &name, int32_t value);
    std::pair<int32_t, Error> GetNumericValue(int id, const std::string &name) const;
    std::pair<std::vector<effects::Parameter>, Error> Parameters(int id) const;
    int Length() const;
    /* len(in) != len(out) is a silent no-op (signal.go:366).  Blocks until the batch this call joined has run. */
    void Process(const double *in, size_t nIn, double *out, size_t nOut, uint32_t sampleRate);

    int channel() const { return channel_; }
private:
    friend class gdg::Engine;
    struct Slot { std::shared_ptr<effects::Unit> unit; bool bypass; };
    Chain(Engine *engine, int channel, const filter::ImpulseResponses *responses) : engine_(engine), channel_(channel), responses_(responses) {}
    Engine *engine_;
    int channel_;
    const filter::ImpulseResponses *responses_;
    mutable std::mutex mutex_;
    std::vector<Slot> slots_;
    uint64_t layoutVersion_ = 1, pushedLayoutVersion_ = 0;
    std::vector<std::shared_ptr<effects::Unit>> retired_;   /* removed units whose device state must be released */
};

/* signal.CreateChain(responses) (signal.go:419-431): the next free channel of the default engine. */
std::shared_ptr<Chain> CreateChain(const filter::ImpulseResponses *responses);

}  // namespace signal

/*
 * One shard of channels on one GPU.  controller.process() has exactly N Chain.Process calls in
 * flight at a time (controller.go:2682-2705, N worker goroutines :3339-3341), so Chain::Process is
 * a rendezvous: every call deposits its buffers, the last arrival launches ONE batched
 * gdg_process_subset for all of them, everybody returns together.  If fewer than the expected
 * number of calls arrive within the timeout, the calls that did arrive are processed as a subset.
 */
class Engine {
public:
    /* one shard (context) per entry of `devices`; channel c lives on shard c * G / N (contiguous blocks).  The same
     * device may be listed more than once (independent contexts): that is how the routing is tested on a one-GPU box. */
    Engine(int nChannels, int maxFrames, std::vector<int> devices);
    Engine(int nChannels, int maxFrames, int device) : Engine(nChannels, maxFrames, std::vector<int>{ device }) {}
    ~Engine();
    static Engine &Default();                              /* configured by Configure() or GDG_CHANNELS / GDG_DEVICES */
    static void Configure(int nChannels, int maxFrames, int device);
    std::pair<std::shared_ptr<signal::Chain>, Error> CreateChain(const filter::ImpulseResponses *responses);
    void SetRendezvous(int expected, int timeoutMs) { expected_ = expected; timeoutMs_ = timeoutMs; }
    /* direct batch call for callers that already hold all channels' buffers (bench, tests) */
    Error ProcessAll(const double *const *in, double *const *out, int frames, uint32_t sampleRate);
    /* controller.processFiles between "the files are read" and "the files are written" (controller.go:2884-3219) over ALL shards:
     * the chains are synchronised to the devices, every shard runs its block of channels on its own thread, `window` blocks per step
     * (gdg_batch_run_shard; shard 0 also runs the metronome), and the master is finished once on shard 0's device: the shards'
     * float64 partial mixes added in shard order, then the metronome as aux input (options.metronome_to_master), then the encoder
     * (gdg_batch_finish_master) -- the reference's sum over all channels -> + aux -> encode (spatializer.go:300-310,
     * controller.go:3123-3219).  inputs: one per channel of the engine; outs: N + 3 host buffers as for gdg_batch_run
     * (NULL = "skipping output"); `samples` receives the length of every output. */
    Error BatchRun(const gdg_batch_input *inputs, int nInputs, const gdg_batch_options &options, int window, void *const *outs, size_t *samples);
    /* BatchRun in slices of whole 8192-sample blocks, files of any length in bounded memory (gdg_batch_stream_open / _need / _step /
     * _close, include/gdg.h): Open synchronises the chains to the device and sets the window, `samples` receives the job's length; Need
     * fills first[i] / count[i] (one per input) with the source frames the next slice of `blocks` blocks must bring; Step takes those
     * frames (ins[i], interleaved, the file's format) and writes the slice's N + 3 output pieces.  The chains must not change between
     * Open and Close.  For an engine of ONE shard: an engine of several shards answers "BatchStream: unsupported ..." (its streamed
     * run is BatchStreamSharded*, below). */
    Error BatchStreamOpen(const gdg_batch_input *inputs, int nInputs, const gdg_batch_options &options, int window, size_t *samples);
    Error BatchStreamNeed(int blocks, size_t *first, size_t *count);
    Error BatchStreamStep(int blocks, const void *const *ins, void *const *outs);
    Error BatchStreamClose();
    /* The streamed run of an engine of ANY shard count, one included: the same caller-side shape (N inputs in, N + 3 output pieces per
     * slice), inside BatchRun's algorithm per slice.  Open synchronises every shard and opens its job at the longest shard's length
     * (gdg_batch_stream_open_shard, the metronome on shard 0); Step runs the shards' slices concurrently, one thread each and shard 0 on
     * the caller's (gdg_batch_stream_step_shard), then finishes the slice's master on shard 0 (gdg_batch_finish_master_slice).  The host
     * holds one slice of partial sums (a pair per shard and the metronome row, blocks * 8192 float64 each), nothing of the job's length.
     * A shard that fails closes every shard's job. */
    Error BatchStreamShardedOpen(const gdg_batch_input *inputs, int nInputs, const gdg_batch_options &options, int window, size_t *samples);
    Error BatchStreamShardedNeed(int blocks, size_t *first, size_t *count);
    Error BatchStreamShardedStep(int blocks, const void *const *ins, void *const *outs);
    Error BatchStreamShardedClose();
    /* No reference counterpart.  The open streamed job as a blob, and a job continued from one (gdg_batch_stream_checkpoint / _resume,
     * include/gdg.h): Checkpoint is valid between any two slices and changes nothing; Resume takes the place of Open on an engine whose
     * chains are set up as for the fresh job -- it synchronises them to the device, sets the window (which may differ from the
     * source's) and opens the job at the recorded position, returned in `samplesDone`.  All or nothing.  The pair without "Sharded" is
     * for an engine of ONE shard, as BatchStreamOpen is.  The sharded pair writes one container per shard behind a small host-side
     * wrapper ("GDGENGCK", version, shard count, slices done, then per shard its size and its container); Resume refuses a wrapper of
     * another shard count, and a shard that rejects its container closes the shards already resumed.  `slicesDone`: the wrapper's. */
    Error BatchStreamCheckpoint(std::vector<uint8_t> &blob);
    Error BatchStreamResume(const gdg_batch_input *inputs, int nInputs, const gdg_batch_options &options, int window, const uint8_t *blob, size_t bytes,
                            size_t *samplesDone);
    Error BatchStreamShardedCheckpoint(std::vector<uint8_t> &blob);
    Error BatchStreamShardedResume(const gdg_batch_input *inputs, int nInputs, const gdg_batch_options &options, int window, const uint8_t *blob,
                                   size_t bytes, size_t *samplesDone, uint64_t *slicesDone = nullptr);
    /* No reference counterpart.  The render report (include/gdg.h, gdg_block_stats): with SetBatchReport(true), BatchRun and every
     * BatchStreamStep / BatchStreamShardedStep keep the records of what the call rendered, [N + 3][blocks] in gdg_batch_run's port order
     * (the N chain outputs, master left, master right, metronome) whatever the shard count: the chain rows come from the shards'
     * reports, put side by side by channel, the master from the finish, the metronome from the shard that ran it.  The switch is read
     * when a job is set up (BatchRun, the Open and Resume calls); it is not part of a checkpoint. */
    void SetBatchReport(bool on) { report_ = on; }
    Error LastBatchReport(std::vector<gdg_block_stats> &records, int *ports, size_t *blocks) const;
    /* No reference counterpart.  The band spectrum (include/gdg.h, gdg_batch_spectrum_enable): with edges set (2 to 33, Hz, finite, >= 0,
     * strictly ascending; an empty vector: off), the same calls keep the power per port, block and band, [N + 3][blocks][bands] in the
     * report's port order and from the report's three sources whatever the shard count.  A refused list leaves the one in force.  Read
     * when a job is set up, like the report's switch; not part of a checkpoint. */
    Error SetBatchSpectrum(const std::vector<double> &edges);
    Error LastBatchSpectrum(std::vector<double> &bands, int *ports, size_t *blocks, int *nBands) const;
    /* No reference counterpart.  The alignment report (include/gdg.h, gdg_batch_align_enable): ref[p] = the port of the job's N + 3 that
     * port p is measured against, -1 for a port that is not measured (an empty vector: off); 1 <= maxLag <= 2048.  The same calls keep
     * [N + 3][blocks] records in the report's port order whatever the shard count.  The engine splits the list per shard when a job is
     * set up: with more than one shard a reference that lives on another shard is refused here (the metronome lives on shard 0), and so
     * is a list that measures or references a master port -- the finish makes the master and carries no alignment records; BatchRun and
     * the BatchStreamSharded calls go through the shard forms at any shard count and refuse such a list when the job is set up (a one-shard
     * engine measures its master through BatchStreamOpen / Step).  A refused list leaves the one in force.  Not part of a checkpoint. */
    Error SetBatchAlign(const std::vector<int> &ref, int maxLag);
    Error LastBatchAlign(std::vector<gdg_block_align> &records, int *ports, size_t *blocks) const;
    /* No reference counterpart.  The true-peak records (include/gdg.h, gdg_batch_true_peak_enable): the same calls keep [N + 3][blocks]
     * records of the 4x oversampled peak in the report's port order whatever the shard count -- chain rows from the shards, the master's
     * two from the finish, the metronome from shard 0.  Read when a job is set up, like the report's switch; not part of a checkpoint. */
    void SetBatchTruePeak(bool on) { truePeak_ = on; }
    Error LastBatchTruePeak(std::vector<gdg_block_true_peak> &records, int *ports, size_t *blocks) const;
    /* No reference counterpart.  Shared sources (include/gdg.h, gdg_batch_set_sources): source[c] = the JOB channel whose input entry channel
     * c reads, one entry per channel of the engine; an empty vector clears the map.  The engine splits the map per shard when a job is set
     * up (BatchRun, the Open and Resume calls).  A map spans one context: a reader whose root lives on another shard is refused here,
     * with a message, and the map in force stays. */
    Error SetBatchSources(const std::vector<int> &source);
    /* No reference counterpart.  Dither of the LPCM outputs (include/gdg.h, gdg_batch_set_dither): TPDF with rounding, the noise of a sample
     * a function of (seed, port, sample index) alone.  The engine gives every shard the job-wide index of its first channel as port_base when
     * a job is set up (BatchRun, the Open and Resume calls) and keeps the master cursor over the slices of a sharded streamed job (a resumed
     * one seeks to the samples done): an engine of any shard count writes the files of one shard.  on = false: the plain encoders. */
    void SetBatchDither(uint64_t seed, bool on = true) { dither_ = on; ditherSeed_ = seed; }
    /* No reference counterpart.  The output trim (include/gdg.h, gdg_batch_set_trim): a gain per output port in front of the encoders, in the
     * job's channel numbers -- chainGain has one entry per channel of the engine (or none: every chain gain 1).  When a job is set up
     * (BatchRun, the Open and Resume calls) every shard gets its own slice of the chain gains; the two master gains and the metronome's
     * go to shard 0's context, which runs the metronome and finishes the master.  Records, meters and float64 partials stay as rendered.
     * A wrong count or a gain that is not finite is refused and the gains in force stay.  All gains 1.0: off. */
    /* the device side of every chain brought up to date at sampleRate without processing anything: a SaveState behind it saves the layout
     * a later LoadState finds, also on an engine that has not processed yet (the two-pass render saves before its first pass) */
    Error SyncChains(uint32_t sampleRate);
    Error SetBatchTrim(const std::vector<double> &chainGain, double masterLeft = 1.0, double masterRight = 1.0, double metronome = 1.0);
    /* No reference counterpart.  The delivery (include/gdg.h, gdg_batch_set_delivery): from the next job on BatchRun and the plain streamed
     * job write every port at 1 / factor of the session rate (factor 1: off, 2 or 4) -- `outs` of samples / factor samples each -- through
     * the reference's decimator on the finished float64 rows.  Records stay those of the session-rate render.  One-shard engines only: the
     * library's shard and master-finish calls refuse a factor, so an engine of more shards refuses it here, as it does blends; a factor
     * other than 1, 2, 4 is refused and the factor in force stays.  The checkpoint calls refuse while a factor is in force. */
    Error SetBatchDelivery(int factor);
    int BatchDelivery() const { return delivery_; }
    /* ... and with the ratio up / down behind the factor (gdg_batch_set_out_ratio): 44.1 kHz from 192 is (4, 147, 160); `outs` of
     * gdg_batch_out_samples(factor, up, down, first, count) samples each.  (factor, 1, 1) is SetBatchDelivery(factor); a ratio the
     * library would refuse is refused here and what is in force stays. */
    Error SetBatchDelivery(int factor, int up, int down);
    void BatchDeliveryRatio(int *up, int *down) const { if (up) *up = deliveryUp_; if (down) *down = deliveryDown_; }
    /* No reference counterpart.  The blend outputs (include/gdg.h, gdg_batch_set_blends): blend b is the weighted sum of its terms -- (job
     * channel, weight) pairs, 1 to 32 of them -- over the chain outputs, in term order, and port N + 3 + b of BatchRun and the plain streamed
     * job; gain: one output gain per blend, or none (every gain 1).  While blends are in force every call's `outs` and every Last* record
     * list have N + 3 + B ports, and SetBatchAlign takes N + 3 or N + 3 + B entries.  Refused with more than one shard: a shard's context
     * holds its own channels only, so a term on another shard's device cannot be summed there, and the library's shard calls refuse blends.
     * BatchRun of a one-shard engine with blends is the library's plain gdg_batch_run.  A refused list leaves the one in force; an empty
     * list: off. */
    Error SetBatchBlends(const std::vector<std::vector<std::pair<int, double>>> &blends, const std::vector<double> &gain = {},
                         const std::vector<std::vector<int>> &delay = {},      /* delay[b][k]: term k of blend b reads its row that many samples back (gdg_batch_set_blends_delayed); none: every delay 0 */
                         const std::vector<std::vector<std::vector<double>>> &taps = {});      /* taps[b][k]: that term's FIR, 0 to 64 finite taps (gdg_batch_set_blends_filtered); none: no term has one */
    int BatchBlends() const { return blendFirst_.empty() ? 0 : (int)blendFirst_.size() - 1; }
    /* No reference counterpart.  The blend fits (include/gdg.h, gdg_batch_fit_enable): per fit a target port and 1 to 8 term ports of the
     * job -- chain outputs, master left, master right, metronome and the blend ports in force.  While fits are in force BatchRun and the plain
     * streamed job keep one gdg_block_fit per fit and block (LastBatchFit: [fits][blocks]) for gdg_blend_weights_from_fit.  Refused with more
     * than one shard, as the blends are and for their reason: the library's shard calls refuse fits, and BatchRun of a one-shard engine with
     * fits is the library's plain gdg_batch_run.  The ports' upper bound is checked when a job is described.  A refused list leaves the one in
     * force; an empty list: off. */
    Error SetBatchFits(const std::vector<std::pair<int, std::vector<int>>> &fits);
    int BatchFits() const { return (int)fitTarget_.size(); }
    Error LastBatchFit(std::vector<gdg_block_fit> &records, int *fits, size_t *blocks) const;
    /* No reference counterpart.  The Gram list (include/gdg.h, gdg_batch_gram_enable): 2 to 512 different ports of the job.  While a list is in
     * force BatchRun and the plain streamed job keep one Gram record per block (LastBatchGram: [blocks][P (P + 1) / 2] doubles) for
     * gdg_blend_pick_from_gram.  Refused with more than one shard, as the fits are and for their reason; BatchRun of a one-shard engine with a
     * list is the library's plain gdg_batch_run.  The ports' upper bound is checked when a job is described.  A refused list leaves the one in
     * force; an empty list: off. */
    Error SetBatchGram(const std::vector<int> &ports);
    int BatchGramPorts() const { return (int)gramPort_.size(); }
    Error LastBatchGram(std::vector<double> &records, int *ports, size_t *blocks) const;
    /* No reference counterpart.  The tap fits (include/gdg.h, gdg_batch_tapfit_enable): per fit a target port, 1 to 4 term ports and 1 to 64 taps
     * per term, at most 128 unknowns, up to 16 fits.  While fits are in force BatchRun and the plain streamed job keep one tap-fit record per
     * block (LastBatchTapFit: [blocks][D] doubles) for gdg_blend_taps_from_tapfit.  Refused with more than one shard, as the fits are and for
     * their reason; BatchRun of a one-shard engine with tap fits is the library's plain gdg_batch_run.  The ports' upper bound is checked when
     * a job is described.  A refused list leaves the one in force; an empty list: off. */
    struct TapFit { int target; std::vector<int> ports; int taps; };
    Error SetBatchTapFits(const std::vector<TapFit> &fits);
    int BatchTapFits() const { return (int)tapFitTarget_.size(); }
    Error LastBatchTapFit(std::vector<double> &records, size_t *blocks, size_t *doublesPerBlock) const;
    /* No reference counterpart.  The transfer list (include/gdg.h, gdg_batch_transfer_enable): up to 16 (port, target) pairs and one group
     * width of 1, 2, 4 .. 64 bins.  While a list is in force BatchRun and the plain streamed job keep one transfer record per block
     * (LastBatchTransfer: [blocks][pairs x (4096 / group + 1) x 4] doubles) for gdg_match_taps_from_transfer.  Refused with more than one
     * shard, as the tap fits are and for their reason; the ports' upper bound is checked when a job is described.  A refused list leaves
     * the one in force; an empty list: off. */
    struct TransferPair { int port; int target; };
    Error SetBatchTransfers(const std::vector<TransferPair> &pairs, int group);
    int BatchTransfers() const { return (int)transferPort_.size(); }
    Error LastBatchTransfer(std::vector<double> &records, size_t *blocks, size_t *doublesPerBlock) const;
    /* No reference counterpart.  The records of the delivered rows (include/gdg.h, DELIVERED RECORDS; gdg_batch_out_records_enable): from the
     * next job on BatchRun and the plain streamed job keep [N + 3 + blends][blocks] gdg_block_delivered records of the rows the encoders read
     * -- behind the delivery in force, in front of the trim and blend gains -- with a true peak that is seamless across blocks.  One-shard
     * engines only: the library's shard and master-finish calls refuse the switch, so an engine of more shards refuses it here.  The
     * checkpoint calls refuse while it is on. */
    Error SetBatchDelivered(bool on);
    bool BatchDelivered() const { return delivered_; }
    Error LastBatchDelivered(std::vector<gdg_block_delivered> &records, int *ports, size_t *blocks) const;
    /* No reference counterpart.  The loudness records (include/gdg.h, LOUDNESS; gdg_batch_loudness_enable): from the next job on BatchRun and
     * the plain streamed job keep, per port and 100 ms hop, the sum of squares of the K-weighted samples of the session-rate rows -- in front of
     * delivery, trim and blend gain.  A small path of its own beside the nine kinds of batch_records.h: the records stay on the device and
     * LastBatchLoudness asks the context for those of its last call or slice, [N + 3 + blends][hops].  One-shard engines only: the library's
     * shard and master-finish calls refuse the switch, so an engine of more shards refuses it here.  The checkpoint calls refuse while it is on. */
    Error SetBatchLoudness(bool on);
    bool BatchLoudness() const { return loudness_; }
    Error LastBatchLoudness(std::vector<double> &records, int *ports, size_t *hops) const;
    /* No reference counterpart.  The state every channel of the engine carries from one call to the next (include/gdg.h, gdg_state_*) as
     * ONE blob: a small engine header, then one gdg_state blob per global channel -- so that an engine with another shard count (another
     * routing of the channels to contexts) can load it.  LoadState first brings the device side of every chain up to date at `sampleRate`
     * (sync: units, parameters, taps, slot lists) and only then loads, so that the next sync finds the taps pushed and leaves the
     * restored convolution alone.  It is all or nothing per channel; a rejected channel keeps its state and the error names it. */
    Error SaveState(std::vector<uint8_t> &blob);
    Error LoadState(const uint8_t *blob, size_t bytes, uint32_t sampleRate);
    std::string LastError() const;
    int channels() const { return nChannels_; }
    int shards() const { return (int)shards_.size(); }
    /* shard of a channel and the channel's index inside it */
    int shardOf(int channel, int *local = nullptr) const;
    void shardRange(int shard, int *first, int *count) const;
    gdg_ctx *context(int shard = 0);                       /* creates the device context on first use */
    std::mutex &shardMutex(int shard);                     /* a context takes one call at a time (include/gdg.h) */
    void setError(const Error &e);                         /* what lastError() returns; also used by the spatializer / tuner twins for per-shard failures */
    const records::RecordStore &batchRecords(records::Kind kind) const { return stores_[kind]; }      /* what LastBatch* hands out of, for the C wrappers */

private:
    friend class signal::Chain;
    struct Pending { signal::Chain *chain; const double *in; double *out; int frames; uint32_t sampleRate; };
    struct Shard { int device = 0, first = 0, count = 0; gdg_ctx *ctx = nullptr; std::mutex mu; };
    void process(signal::Chain *chain, const double *in, double *out, int frames, uint32_t sampleRate);
    void runBatch(std::vector<Pending> batch);
    Error runShard(int shard, std::vector<Pending> &group, int frames, uint32_t sampleRate);
    Error sync(int shard, const std::vector<signal::Chain *> &chains, uint32_t sampleRate);
    Error prepareShards(const gdg_batch_input *inputs, const gdg_batch_options &options, int window, size_t *jobSamples);   /* chains synced, window set, the job's length */
    int nChannels_, maxFrames_;
    std::vector<std::unique_ptr<Shard>> shards_;
    std::vector<std::shared_ptr<signal::Chain>> chains_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::vector<Pending> pending_;
    bool executing_ = false;
    uint64_t generation_ = 0;
    int expected_ = 0, timeoutMs_ = 50;
    bool shardedOpen_ = false;                             /* BatchStreamSharded*: a job is open on every shard, with these options */
    gdg_batch_options shardedOptions_ = {};
    uint64_t shardedSlices_ = 0;                           /* ... and this many slices done (a checkpoint's wrapper records it) */
    void closeSharded();
    records::RecordStore stores_[records::KINDS];          /* the last batch call's records, one store per kind (batch_records.h) */
    records::Expect expected(records::Kind kind) const;              /* whether the settings in force keep a kind, and at which counts */
    bool report_ = false;                                  /* the render report: asked for */
    std::vector<double> spectrumEdges_;                    /* the band spectrum: the edges in force (empty: off) */
    int applySpectrum(gdg_ctx *ctx);
    std::vector<int> alignRef_;                            /* the alignment report: the list in force over the job's N + 3 ports (empty: off) ... */
    int alignLag_ = 0;                                     /* ... and its lag range */
    int shardOfPort(int port);
    Error alignOverShards(int minShards);
    int applyAlign(int shard, gdg_ctx *ctx);               /* shard < 0: the plain form's list */
    bool truePeak_ = false;                                /* the true-peak records: asked for */
    std::vector<int> sources_;                             /* the source map in job channel numbers; empty: none */
    int applySources(int shard, gdg_ctx *ctx);             /* the shard's part of it onto its context: a gdg_* status */
    bool dither_ = false;                                  /* SetBatchDither: on, and the seed */
    uint64_t ditherSeed_ = 0;
    int applyDither(int shard, gdg_ctx *ctx);              /* mode, seed and the shard's port_base onto its context: a gdg_* status */
    std::vector<double> trim_;                             /* SetBatchTrim: N chain gains, master left, master right, metronome; empty: off */
    int delivery_ = 1;                                     /* SetBatchDelivery: 1 = off; never another value on an engine of several shards */
    int deliveryUp_ = 1, deliveryDown_ = 1;                /* ... and the ratio behind it: 1 / 1 = none; never another on an engine of several shards */
    int applyTrim(int shard, gdg_ctx *ctx);                /* the shard's slice of it onto its context: a gdg_* status */
    std::vector<int> blendFirst_, blendChannel_;           /* SetBatchBlends, in gdg_batch_set_blends' CSR form; blendFirst_ empty: off */
    std::vector<double> blendWeight_, blendGain_;
    std::vector<int> blendDelay_;                          /* one per term, or empty: every delay 0 and the list goes through gdg_batch_set_blends */
    std::vector<int> blendTapFirst_;                       /* one offset per term and one more into blendTap_, or empty: no term has taps and the list goes the delayed way */
    std::vector<double> blendTap_;
    std::vector<int> fitFirst_, fitPort_, fitTarget_;      /* SetBatchFits, in gdg_batch_fit_enable's CSR form; fitTarget_ empty: off */
    int applyFits(gdg_ctx *ctx);                           /* onto a context (more shards: none are in force): a gdg_* status */
    std::vector<int> gramPort_;                            /* SetBatchGram; empty: off */
    int applyGram(gdg_ctx *ctx);                           /* onto a context (more shards: none is in force): a gdg_* status */
    std::vector<int> tapFitFirst_, tapFitPort_, tapFitTarget_, tapFitTaps_;      /* SetBatchTapFits, in the CSR form of the C call; no target: off */
    std::vector<int> transferPort_, transferTarget_;      /* SetBatchTransfers; no pair: off */
    int transferGroup_ = 1;
    bool delivered_ = false;                               /* SetBatchDelivered; never on on an engine of several shards */
    int applyTransfers(gdg_ctx *ctx);                      /* onto a context (more shards: none is in force): a gdg_* status */
    int applyTapFits(gdg_ctx *ctx);                        /* onto a context (more shards: none are in force): a gdg_* status */
    bool loudness_ = false;                                /* SetBatchLoudness; never on on an engine of several shards */
    bool plainRun() const { return BatchBlends() > 0 || BatchFits() > 0 || BatchGramPorts() > 0 || BatchTapFits() > 0 || BatchTransfers() > 0 || delivered_ || loudness_ || delivery_ > 1 || deliveryUp_ != 1 || deliveryDown_ != 1; }      /* BatchRun is the library's plain one-call run */
    int applyBlends(gdg_ctx *ctx);                         /* onto the one context of a one-shard engine (more shards: none are in force): a gdg_* status */
    /* every setting in force onto a context, in the order the library's checks need: the window, the four port kinds, sources, dither,
     * trim, delivery and blends (applyPortSettings: all that a resumed job is set up with), then the five list kinds.  shard < 0: the plain
     * form of a one-shard engine, whose alignment list covers the master and the blend ports.  A gdg_* status */
    int applyPortSettings(int shard, gdg_ctx *ctx, int window);
    int applySettings(int shard, gdg_ctx *ctx, int window);
    int ports() const { return nChannels_ + 3 + BatchBlends(); }      /* of a batch call: N + 3 and the blends in force */
    Error recordsOfContext(gdg_ctx *ctx);                  /* one shard, the plain run: the context's records of every kind are the engine's */
    void reportBegin(size_t blocks);
    Error reportOfShard(int shard, gdg_ctx *ctx);
    Error reportOfMaster(gdg_ctx *ctx);
    mutable std::mutex errMu_;
    std::string lastError_;
};

/* ---- spatializer.Spatializer (spatializer/spatializer.go:30-41): the ten methods, on top of an engine's shards -------------
 * Every shard mixes its block of channels to a partial (left, right) pair; the host adds the partials in shard order and then the
 * aux input (spatializer.go:300-310).  Error strings are the reference's. */
namespace spatializer {
constexpr uint32_t OUTPUT_COUNT = 2;
class Spatializer {
public:
    Spatializer(Engine *engine, uint32_t inputChannels);
    std::pair<double, Error> GetAzimuth(uint32_t inputChannel) const;
    std::pair<double, Error> GetDistance(uint32_t inputChannel) const;
    std::pair<double, Error> GetLevel(uint32_t inputChannel) const;
    uint32_t GetInputCount() const { return inputCount_; }
    uint32_t GetOutputCount() const { return OUTPUT_COUNT; }
    /* inputBuffers: inputCount rows of n samples; auxInputBuffer may be null; outputBuffers: 2 rows of n samples.
     * reuseChainOutputs: the inputs ARE the outputs of the engine's last block (what controller.process() passes,
     * controller.go:2744-2761) and are still on the devices: nothing is uploaded. */
    void Process(const double *const *inputBuffers, const double *auxInputBuffer, double *const *outputBuffers, size_t n, bool reuseChainOutputs = false);
    Error SetAzimuth(uint32_t inputChannel, double azimuth);
    Error SetDistance(uint32_t inputChannel, double distance);
    Error SetLevel(uint32_t inputChannel, double level);
    void SetSampleRate(uint32_t rate);
private:
    void push(uint32_t channel);
    Engine *engine_;
    uint32_t inputCount_;
    mutable std::mutex mutex_;
    struct Position { double azimuth = 0.0, distance = 0.0, level = 1.0; };
    std::vector<Position> positions_;
};
std::shared_ptr<Spatializer> Create(Engine *engine, uint32_t inputChannels);       /* spatializer.go:436-469 */
}  // namespace spatializer

/* ---- tuner.Tuner (tuner/tuner.go:62-65): Process enqueues, Analyze runs the 262144-point autocorrelation on the device ---- */
namespace tuner {
struct Result { int8_t cents; double frequency; std::string note; };              /* tuner.go:30-46 */
class Tuner {
public:
    explicit Tuner(int device);
    ~Tuner();
    std::pair<Result, Error> Analyze();
    void Process(const double *samples, size_t n, uint32_t sampleRate);
private:
    /* the reference's two locks (tuner.go:48-57): Process -- the audio path -- only ever takes mutexBuffer_ for one enqueue into the host ring;
     * Analyze owns the device context under mutexAnalyze_ and holds mutexBuffer_ (shared) just while it copies the ring out (tuner.go:408-412) */
    std::shared_mutex mutexBuffer_;
    std::vector<double> ring_;             /* circular.Buffer of NUM_SAMPLES (circular.go:33-105) */
    size_t pointer_ = 0;
    uint32_t sampleRate_ = 0;
    std::mutex mutexAnalyze_;
    std::vector<double> snapshot_;         /* the ring, oldest sample first */
    gdg_ctx *ctx_ = nullptr;
    int device_;
};
std::shared_ptr<Tuner> Create(int device = 0);                                     /* tuner.go:592-610 */
}  // namespace tuner

}  // namespace gdg

#endif
