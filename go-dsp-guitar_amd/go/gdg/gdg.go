// Package gdg is the thin cgo binding of libgdg.so (include/gdg.h): the MI355X-native batch
// implementation of go-dsp-guitar's per-channel effects pipeline.
//
// NOT compiled in the authoring container (no Go toolchain there); it is the directory a maintainer copies into the reference
// checkout as <ref>/gdg (package github.com/andrepxx/go-dsp-guitar/gdg, INTEGRATION.md section 3 -- cgo needs the package
// directory on disk, an overlay-only directory will not do).  Written for the language level of the reference's go.mod (go 1.16):
// no unsafe.Slice / unsafe.Add, no generics, no `any`, no typed atomics (tests/test_go_sources.py holds the deny-list).
// It contains no DSP: every function is one C call.
//
//	CGO_CFLAGS="-I<repo>/include" CGO_LDFLAGS="-L<repo>/go-dsp-guitar_amd/lib -lgdg -Wl,-rpath,<repo>/go-dsp-guitar_amd/lib"
package gdg

/*
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "gdg.h"
*/
import "C"

import (
	"fmt"
	"os"
	"strconv"
	"strings"
	"sync"
	"unsafe"
)

// Context is one shard of channels on one GPU (gdg_ctx).  A context takes ONE call at a time (include/gdg.h): callers that
// share it serialise on Shard.Mutex.
type Context struct {
	ctx      *C.gdg_ctx
	in       unsafe.Pointer // pinned host slab, row c = channel c (gdg_staging_buffers)
	out      unsafe.Pointer
	stride   int
	channels int
	scratch  unsafe.Pointer // C memory for MetersProcess: [ports pointers | ports x frames float64]
	scratchN int
	// the streamed batch run that is open (BatchStreamOpen): its inputs and the width of an output sample
	streamInputs int
	streamWidth  int
	streamDone   int // session samples of the open streamed job's slices so far: what a delivery ratio counts a slice's samples from
}

// DeviceCount: HIP devices visible to the process (0 without a driver).
func DeviceCount() int { return int(C.gdg_device_count()) }

func (this *Context) err(rc C.int) error {
	if rc == C.GDG_OK {
		return nil
	}
	return fmt.Errorf("gdg: %s (code %d)", C.GoString(C.gdg_last_error(this.ctx)), int(rc))
}

// CreateContext replaces N x signal.CreateChain + spatializer.Create + tuner.Create for one shard
// (controller/controller.go:3267-3279).
func CreateContext(channels int, maxFrames int, device int) (*Context, error) {
	c := &Context{}
	rc := C.gdg_ctx_create(C.int(channels), C.int(maxFrames), C.int(device), &c.ctx)
	if rc != C.GDG_OK {
		return nil, fmt.Errorf("gdg_ctx_create failed with code %d (no usable HIP device; there is no CPU fallback)", int(rc))
	}
	var in, out *C.double
	var stride C.int
	if err := c.err(C.gdg_staging_buffers(c.ctx, &in, &out, &stride)); err != nil {
		return nil, err
	}
	c.in, c.out, c.stride, c.channels = unsafe.Pointer(in), unsafe.Pointer(out), int(stride), channels
	return c, nil
}

func (this *Context) Destroy() {
	if this.scratch != nil {
		C.free(this.scratch)
		this.scratch = nil
	}
	C.gdg_ctx_destroy(this.ctx)
}

func (this *Context) Channels() int  { return this.channels }
func (this *Context) MaxFrames() int { return this.stride }

// UnitCreate: effects.CreateUnit(unitType) on the device side (effects/effects.go:443-516).
func (this *Context) UnitCreate(channel int, unitType int) (int, error) {
	var h C.int
	err := this.err(C.gdg_unit_create(this.ctx, C.int(channel), C.int(unitType), &h))
	return int(h), err
}

func (this *Context) UnitDestroy(handle int) error {
	return this.err(C.gdg_unit_destroy(this.ctx, C.int(handle)))
}

// UnitSetParam passes one RESOLVED parameter: the int32 of a numeric parameter or the index of a
// discrete value.  Name lookup and range checks stay in the reference's effects package.
func (this *Context) UnitSetParam(handle int, index int, value int32) error {
	return this.err(C.gdg_unit_set_param(this.ctx, C.int(handle), C.int(index), C.int32_t(value)))
}

// UnitSetFir hands over the composite taps of a power amp (what poweramp.compile() returns).
func (this *Context) UnitSetFir(handle int, taps []float64) error {
	var p *C.double
	if len(taps) > 0 {
		p = (*C.double)(unsafe.Pointer(&taps[0])) // a []float64 holds no Go pointers: legal for the duration of the call
	}
	return this.err(C.gdg_unit_set_fir(this.ctx, C.int(handle), p, C.int(len(taps))))
}

// UnitCompileFir runs poweramp.compile() on the device (effects/poweramp.go:25-127): slot i = taps of impulse response i at the
// current rate (nil = "- NONE -"), its gain compensation factor and its level in dB.  An array of Go slices would be a
// pointer to Go pointers, which cgo forbids, so every slot is copied into C memory for the duration of the call.
func (this *Context) UnitCompileFir(handle int, taps [][]float64, compensation []float64, levelsDb []int32, targetOrder uint32) error {
	n := len(taps)
	if n == 0 {
		return this.err(C.gdg_unit_compile_fir(this.ctx, C.int(handle), 0, nil, nil, nil, nil, C.uint32_t(targetOrder)))
	}
	ptrSize := C.size_t(unsafe.Sizeof(uintptr(0)))
	ptrs := (*[1 << 20]*C.double)(C.calloc(C.size_t(n), ptrSize))
	defer C.free(unsafe.Pointer(ptrs))
	lens := make([]C.int, n)
	comp := make([]C.double, n)
	lev := make([]C.int32_t, n)
	for i := 0; i < n; i++ {
		comp[i] = C.double(compensation[i])
		lev[i] = C.int32_t(levelsDb[i])
		if len(taps[i]) == 0 {
			continue
		}
		bytes := C.size_t(len(taps[i])) * 8
		mem := C.malloc(bytes)
		defer C.free(mem)
		C.memcpy(mem, unsafe.Pointer(&taps[i][0]), bytes)
		ptrs[i] = (*C.double)(mem)
		lens[i] = C.int(len(taps[i]))
	}
	return this.err(C.gdg_unit_compile_fir(this.ctx, C.int(handle), C.int(n), (**C.double)(unsafe.Pointer(ptrs)), &lens[0], &comp[0], &lev[0], C.uint32_t(targetOrder)))
}

func (this *Context) ChainSet(channel int, handles []int, bypass []bool) error {
	n := len(handles)
	hs := make([]C.int, n+1)
	bs := make([]C.uint8_t, n+1)
	for i := 0; i < n; i++ {
		hs[i] = C.int(handles[i])
		if bypass[i] {
			bs[i] = 1
		}
	}
	return this.err(C.gdg_chain_set(this.ctx, C.int(channel), &hs[0], &bs[0], C.int(n)))
}

// ---- channel state: no reference counterpart (include/gdg.h, gdg_state_*) ----------------------------------------------

// stateChannels: the channel list of a gdg_state_* call (nil = every channel in order, the pointer then stays nil).
func stateChannels(channels []int) (*C.int, C.int) {
	if channels == nil {
		return nil, 0
	}
	cs := make([]C.int, len(channels)+1) // one spare element: &cs[0] of an empty list is still valid
	for i, c := range channels {
		cs[i] = C.int(c)
	}
	return &cs[0], C.int(len(channels))
}

// SaveState returns what the listed channels (nil: all, in order) carry from one call to the next, one record per channel.  The
// context is not changed: a stream with saves between its calls gives the same samples.  A runShard that fails can load the last
// good blob back instead of resetting every unit of the shard.
func (this *Context) SaveState(channels []int) ([]byte, error) {
	pc, n := stateChannels(channels)
	var size C.size_t
	if err := this.err(C.gdg_state_size(this.ctx, pc, n, &size)); err != nil {
		return nil, err
	}
	buf := make([]byte, int(size)+1)
	var written C.size_t
	if err := this.err(C.gdg_state_save(this.ctx, pc, n, unsafe.Pointer(&buf[0]), size, &written)); err != nil {
		return nil, err
	}
	return buf[:int(written)], nil
}

// LoadState applies record i of blob to channels[i] (nil: every channel in order; the count must be the blob's).  All or
// nothing: a blob that does not fit the channels' chains is an error and changes nothing.
func (this *Context) LoadState(channels []int, blob []byte) error {
	if len(blob) == 0 {
		return fmt.Errorf("gdg: an empty state blob")
	}
	pc, n := stateChannels(channels)
	return this.err(C.gdg_state_load(this.ctx, pc, n, unsafe.Pointer(&blob[0]), C.size_t(len(blob))))
}

// Row returns channel c's rows of the pinned staging slabs as Go slices over C memory.  The slab has `channels` rows of
// `stride` (= max_frames) float64: anything outside is an error, never a slice (a longer slice would run into the next
// channel's row and, for the last channel, past the hipHostMalloc slab).
func (this *Context) Row(channel int, frames int) (in []float64, out []float64, err error) {
	if channel < 0 || channel >= this.channels {
		return nil, nil, fmt.Errorf("gdg: channel %d out of range (the context has %d)", channel, this.channels)
	}
	if frames < 0 || frames > this.stride {
		return nil, nil, fmt.Errorf("gdg: %d frames do not fit a staging row of %d", frames, this.stride)
	}
	// slices over C memory the Go 1.16 way (the reference's go.mod:3 says `go 1.16`; unsafe.Slice is 1.17): a pointer to a
	// huge array type, sliced down to the row with its capacity capped
	off := uintptr(channel) * uintptr(this.stride) * 8
	in = (*[1 << 37]float64)(unsafe.Pointer(uintptr(this.in) + off))[:frames:frames]
	out = (*[1 << 37]float64)(unsafe.Pointer(uintptr(this.out) + off))[:frames:frames]
	return in, out, nil
}

// ProcessStaged runs the chains of the listed channels on the frames deposited in the staging rows.
func (this *Context) ProcessStaged(channels []int, frames int, sampleRate uint32) error {
	if len(channels) == 0 {
		return nil // nothing to run; &cs[0] of an empty slice would panic
	}
	cs := make([]C.int, len(channels))
	for i, c := range channels {
		cs[i] = C.int(c)
	}
	return this.err(C.gdg_process_staged(this.ctx, &cs[0], C.int(len(cs)), C.int(frames), C.uint32_t(sampleRate)))
}

// ---- tuner: tuner.Process / tuner.Analyze (tuner/tuner.go:379-587) ------------------------------------------------

type TunerResult struct {
	Frequency float64
	NoteIndex int // index into the 61-note table, -1 = "Unknown"
	Cents     int8
}

// TunerEnqueueStaged: tuner.Process for every channel of the context from the pinned INPUT rows (fill them through Row).
func (this *Context) TunerEnqueueStaged(frames int, sampleRate uint32) error {
	return this.err(C.gdg_tuner_enqueue_staged(this.ctx, C.int(frames), C.uint32_t(sampleRate)))
}

// TunerReplace: the whole ring of one channel at once -- len(samples) must be the ring's length (tuner.NUM_SAMPLES = 96000, oldest
// sample first: what circular.Buffer.Retrieve hands out); anything else is an error from the library, never a partial upload.
func (this *Context) TunerReplace(channel int, samples []float64, sampleRate uint32) error {
	if len(samples) == 0 {
		return fmt.Errorf("gdg: an empty ring")
	}
	return this.err(C.gdg_tuner_replace(this.ctx, C.int(channel), (*C.double)(unsafe.Pointer(&samples[0])), C.int(len(samples)), C.uint32_t(sampleRate)))
}

// TunerAnalyze: tuner.Analyze for every channel of the context.
func (this *Context) TunerAnalyze() ([]TunerResult, error) {
	n := this.channels
	raw := (*[1 << 20]C.gdg_tuner_result)(C.calloc(C.size_t(n), C.size_t(unsafe.Sizeof(C.gdg_tuner_result{}))))
	defer C.free(unsafe.Pointer(raw))
	if err := this.err(C.gdg_tuner_analyze(this.ctx, &raw[0])); err != nil {
		return nil, err
	}
	res := make([]TunerResult, n)
	for i := 0; i < n; i++ {
		res[i] = TunerResult{Frequency: float64(raw[i].frequency), NoteIndex: int(raw[i].note_index), Cents: int8(raw[i].cents)}
	}
	return res, nil
}

// TunerNoteName: name of a note of the reference's table (tuner/tuner.go:79-324), "Unknown" for -1.
func TunerNoteName(index int) string { return C.GoString(C.gdg_tuner_note_name(C.int(index))) }

// ---- spatializer: partial N -> 2 mix of this shard (spatializer/spatializer.go:140-335) -----------------------------

func (this *Context) SpatializerSetPosition(channel int, azimuth float64, distance float64, level float64) error {
	return this.err(C.gdg_spatializer_set_position(this.ctx, C.int(channel), C.double(azimuth), C.double(distance), C.double(level)))
}

func (this *Context) SpatializerSetSampleRate(rate uint32) error {
	return this.err(C.gdg_spatializer_set_sample_rate(this.ctx, C.uint32_t(rate)))
}

// SpatializeStaged mixes this shard's channels into left / right (len = frames).  fromOutputs: the inputs are the chain outputs
// of the last ProcessStaged over ALL channels of the context, still on the device (nothing is uploaded); otherwise the pinned
// INPUT rows.  left / right are []float64 (no Go pointers inside): legal cgo arguments for the duration of the call.
func (this *Context) SpatializeStaged(fromOutputs bool, left []float64, right []float64) error {
	if len(left) == 0 || len(left) != len(right) {
		return fmt.Errorf("gdg: bad output buffers")
	}
	f := C.int(0)
	if fromOutputs {
		f = 1
	}
	return this.err(C.gdg_spatialize_staged(this.ctx, f, (*C.double)(unsafe.Pointer(&left[0])), (*C.double)(unsafe.Pointer(&right[0])), C.int(len(left))))
}

// ---- shards: one context per GPU, channel c on shard c * G / N (contiguous blocks; SURVEY.md 8e, controller.go:3262-3269) ----

type Shard struct {
	Ctx    *Context
	Device int
	First  int // first global channel of the block
	Count  int
	Mutex  sync.Mutex // one call at a time per context
}

var (
	shardMutex sync.Mutex
	shardList  []*Shard
	shardTotal int
)

// devices: GDG_DEVICES="0,1,2,..." (one shard per entry; an entry may repeat), else GDG_DEVICE, else every visible device.
func devices() []int {
	if list := os.Getenv("GDG_DEVICES"); list != "" {
		var devs []int
		for _, item := range strings.Split(list, ",") {
			if d, err := strconv.Atoi(strings.TrimSpace(item)); err == nil {
				devs = append(devs, d)
			}
		}
		if len(devs) > 0 {
			return devs
		}
	}
	if one := os.Getenv("GDG_DEVICE"); one != "" {
		d, _ := strconv.Atoi(one)
		return []int{d}
	}
	n := DeviceCount()
	if n < 1 {
		n = 1
	}
	devs := make([]int, n)
	for i := range devs {
		devs[i] = i
	}
	return devs
}

// Shards creates (once) the contexts for a job of totalChannels channels and returns them.  The same algorithm as
// gdg::Engine::Engine in host/gdg_host.cpp: never more shards than channels, shard g owns [g N / G, (g + 1) N / G).
func Shards(totalChannels int, maxFrames int) ([]*Shard, error) {
	shardMutex.Lock()
	defer shardMutex.Unlock()
	if shardList != nil {
		if totalChannels > shardTotal {
			return nil, fmt.Errorf("gdg: the shards were created for %d channels, %d requested", shardTotal, totalChannels)
		}
		return shardList, nil
	}
	devs := devices()
	G := len(devs)
	if G > totalChannels {
		G = totalChannels
	}
	if G < 1 {
		G = 1
	}
	list := make([]*Shard, 0, G)
	for g := 0; g < G; g++ {
		first := g * totalChannels / G
		count := (g+1)*totalChannels/G - first
		ctx, err := CreateContext(count, maxFrames, devs[g])
		if err != nil {
			for _, sh := range list {
				sh.Ctx.Destroy()
			}
			return nil, err
		}
		list = append(list, &Shard{Ctx: ctx, Device: devs[g], First: first, Count: count})
	}
	shardList, shardTotal = list, totalChannels
	return shardList, nil
}

// ShardOf: the shard of a global channel and the channel's index inside it (nil before Shards() or out of range).
func ShardOf(channel int) (*Shard, int) {
	shardMutex.Lock()
	defer shardMutex.Unlock()
	for _, sh := range shardList {
		if channel >= sh.First && channel < sh.First+sh.Count {
			return sh, channel - sh.First
		}
	}
	return nil, -1
}

// ---- the data formats either side of the chain (optional; include/gdg.h "data formats" section) ----------------

// WaveDecode: bytesToSamples + samplesToChannels (wave/wave.go:237-270, :790-838).  data = the data chunk of a RIFF/WAVE file
// (a []byte holds no Go pointers: legal for the duration of the call); returns planar samples, one slice per channel.
func (this *Context) WaveDecode(format int, data []byte, channels int) ([][]float64, error) {
	width := int(C.gdg_wave_bytes_per_sample(C.int(format)))
	if width == 0 || channels <= 0 {
		return nil, fmt.Errorf("gdg: unknown sample format %d or bad channel count %d", format, channels)
	}
	per := len(data) / (width * channels)
	flat := make([]float64, per*channels)
	if per > 0 {
		rc := C.gdg_wave_decode(this.ctx, C.int(format), unsafe.Pointer(&data[0]), C.size_t(per), C.uint(channels), (*C.double)(unsafe.Pointer(&flat[0])))
		if err := this.err(rc); err != nil {
			return nil, err
		}
	}
	out := make([][]float64, channels)
	for c := range out {
		out[c] = flat[c*per : (c+1)*per]
	}
	return out, nil
}

// WaveEncode: channelsToSamples + samplesToBytes (wave/wave.go:173-232, :737-785) of equally long channels.
func (this *Context) WaveEncode(format int, channels [][]float64) ([]byte, error) {
	width := int(C.gdg_wave_bytes_per_sample(C.int(format)))
	if width == 0 || len(channels) == 0 {
		return nil, fmt.Errorf("gdg: unknown sample format %d or no channels", format)
	}
	per := len(channels[0])
	flat := make([]float64, 0, per*len(channels))
	for _, ch := range channels {
		flat = append(flat, ch[:per]...)
	}
	data := make([]byte, per*len(channels)*width)
	if per == 0 {
		return data, nil
	}
	rc := C.gdg_wave_encode(this.ctx, C.int(format), (*C.double)(unsafe.Pointer(&flat[0])), C.size_t(per), C.uint(len(channels)), unsafe.Pointer(&data[0]))
	return data, this.err(rc)
}

// ResampleTime: resample.Time (resample/resample.go:72-103).
func (this *Context) ResampleTime(samples []float64, sourceRate uint32, targetRate uint32) ([]float64, error) {
	n := C.gdg_resample_time_length(C.int(len(samples)), C.uint32_t(sourceRate), C.uint32_t(targetRate))
	if n <= 0 || len(samples) == 0 {
		return []float64{}, nil
	}
	out := make([]float64, int(n))
	rc := C.gdg_resample_time(this.ctx, (*C.double)(unsafe.Pointer(&samples[0])), C.int(len(samples)), C.uint32_t(sourceRate), C.uint32_t(targetRate),
		(*C.double)(unsafe.Pointer(&out[0])), n)
	return out, this.err(rc)
}

// MetersConfigure / MetersSetEnabled / MetersAnalyze: level.Meter over n ports (level/level.go:100-279).  Buffers reach the meters
// through MetersProcessDevice on rows already resident on the device (the staging slab's device twin) or through
// gdg_meter_process with C-allocated rows; Go slices of slices cannot cross cgo.
func (this *Context) MetersConfigure(ports int) error { return this.err(C.gdg_meter_configure(this.ctx, C.int(ports))) }
func (this *Context) MetersSetEnabled(port int, enabled bool) error {
	e := C.int(0)
	if enabled {
		e = 1
	}
	return this.err(C.gdg_meter_set_enabled(this.ctx, C.int(port), e))
}

// MetersProcess: level.Meter.Process over `buffers` (one per port, level/level.go:302-325).  A [][]float64 is a pointer to Go
// pointers and cannot cross cgo, so the buffers are copied into C memory owned by the context.
func (this *Context) MetersProcess(buffers [][]float64, sampleRate uint32) error {
	ports := len(buffers)
	if ports == 0 {
		return nil
	}
	frames := len(buffers[0])
	ptrBytes := ports * int(unsafe.Sizeof(uintptr(0)))
	need := ptrBytes + ports*frames*8
	if need > this.scratchN {
		if this.scratch != nil {
			C.free(this.scratch)
		}
		this.scratch = C.malloc(C.size_t(need))
		this.scratchN = need
	}
	ptrs := (*[1 << 20]*C.double)(this.scratch)
	data := unsafe.Pointer(uintptr(this.scratch) + uintptr(ptrBytes))
	for p, buf := range buffers {
		if len(buf) != frames {
			return fmt.Errorf("gdg: meter buffers must be of equal length")
		}
		row := unsafe.Pointer(uintptr(data) + uintptr(p*frames*8))
		if frames > 0 {
			C.memcpy(row, unsafe.Pointer(&buf[0]), C.size_t(frames*8))
		}
		ptrs[p] = (*C.double)(row) // a C pointer stored in C memory: allowed
	}
	return this.err(C.gdg_meter_process(this.ctx, (**C.double)(this.scratch), C.int(frames), C.uint32_t(sampleRate)))
}

func (this *Context) MetersAnalyze(ports int) (levels []int32, peaks []int32, err error) {
	levels, peaks = make([]int32, ports), make([]int32, ports)
	if ports == 0 {
		return levels, peaks, nil
	}
	err = this.err(C.gdg_meter_analyze(this.ctx, (*C.int32_t)(unsafe.Pointer(&levels[0])), (*C.int32_t)(unsafe.Pointer(&peaks[0]))))
	return levels, peaks, err
}

// Metronome: metronome.Metronome (metronome/metronome.go:63-131).
func (this *Context) MetronomeSetTick(coefficients []float64) error {
	if coefficients == nil {
		return this.err(C.gdg_metronome_set_tick(this.ctx, nil, 0))
	}
	var dummy C.double
	p := &dummy
	if len(coefficients) > 0 {
		p = (*C.double)(unsafe.Pointer(&coefficients[0]))
	}
	return this.err(C.gdg_metronome_set_tick(this.ctx, p, C.int(len(coefficients))))
}
func (this *Context) MetronomeSetTock(coefficients []float64) error {
	if coefficients == nil {
		return this.err(C.gdg_metronome_set_tock(this.ctx, nil, 0))
	}
	var dummy C.double
	p := &dummy
	if len(coefficients) > 0 {
		p = (*C.double)(unsafe.Pointer(&coefficients[0]))
	}
	return this.err(C.gdg_metronome_set_tock(this.ctx, p, C.int(len(coefficients))))
}
func (this *Context) MetronomeConfigure(beatsPerPeriod uint32, bpmSpeed uint32, sampleRate uint32) error {
	return this.err(C.gdg_metronome_configure(this.ctx, C.uint32_t(beatsPerPeriod), C.uint32_t(bpmSpeed), C.uint32_t(sampleRate)))
}
func (this *Context) MetronomeProcess(out []float64) error {
	if len(out) == 0 {
		return nil
	}
	return this.err(C.gdg_metronome_process(this.ctx, (*C.double)(unsafe.Pointer(&out[0])), C.int(len(out))))
}

// SetWindow: the batch run steps through the files `frames` (1, 2, 4, 8 or 16) blocks at a time; every power amp then reads its IR
// spectra and its delay line once per step instead of once per block (gdg_ctx_set_window).
func (this *Context) SetWindow(frames int) error {
	return this.err(C.gdg_ctx_set_window(this.ctx, C.int(frames)))
}

// SetOverlap: free-running channel groups of the device-resident calls, opt-in (gdg_ctx_set_overlap: 0 or 1 = one group on the
// context's stream, the default; > 1: groups on streams of their own, joined by the next call of any other kind).
func (this *Context) SetOverlap(groups int) error {
	return this.err(C.gdg_ctx_set_overlap(this.ctx, C.int(groups)))
}

// SetOption / Option: the library's launch-shape options (gdg_ctx_set_option in include/gdg.h lists the keys) -- what used to be
// environment variables of the process.  The drop-in needs none of them; they are here for deployments that tune a node
// ("numa", "copy_threads", "seg_wave_max_channels", ...).
func (this *Context) SetOption(key string, value int64) error {
	k := C.CString(key)
	defer C.free(unsafe.Pointer(k))
	return this.err(C.gdg_ctx_set_option(this.ctx, k, C.longlong(value)))
}
func (this *Context) Option(key string) (int64, error) {
	k := C.CString(key)
	defer C.free(unsafe.Pointer(k))
	var v C.longlong
	if e := this.err(C.gdg_ctx_get_option(this.ctx, k, &v)); e != nil {
		return 0, e
	}
	return int64(v), nil
}

// BatchInput: one input file of the batch run -- the data section of a RIFF/WAVE file (wave.go:840-1100 parses the header and
// knows Format / BitDepth / SampleRate / ChannelCount), and the channel of it that feeds the input.  Data == nil leaves the
// channel empty (controller.go:2935).
type BatchInput struct {
	Data       []byte
	Format     int // gdg_wave_format
	SampleRate uint32
	Channels   int
	Channel    int
}

type BatchOptions struct {
	TargetRate        uint32
	OutFormat         int
	MetronomeToMaster bool
	RunMeters         bool
	TunerEnqueue      bool
}

func cbool(b bool) C.int {
	if b {
		return 1
	}
	return 0
}

// BatchRun: controller.processFiles between "the files are read" and "the files are written" (controller/controller.go:2884-3219)
// in one call.  The C structs hold pointers, so the file bytes live in C memory for the duration of the call (C.CBytes: one copy), and so do the N + 3 output data sections.
func (this *Context) BatchRun(inputs []BatchInput, opt BatchOptions) ([][]byte, error) {
	n := len(inputs)
	if n == 0 {
		return nil, fmt.Errorf("gdg: no inputs")
	}
	arr, release, err := batchInputs(inputs)
	if err != nil {
		return nil, err
	}
	defer release()
	var owned []unsafe.Pointer
	defer func() {
		for _, p := range owned {
			C.free(p)
		}
	}()
	o := C.gdg_batch_options{target_rate: C.uint32_t(opt.TargetRate), out_format: C.int(opt.OutFormat),
		metronome_to_master: cbool(opt.MetronomeToMaster), run_meters: cbool(opt.RunMeters), tuner_enqueue: cbool(opt.TunerEnqueue)}
	var samples C.size_t
	if e := this.err(C.gdg_batch_length(this.ctx, &arr[0], C.int(n), o.target_rate, &samples)); e != nil {
		return nil, e
	}
	each := this.delivered(0, int(samples)) * int(C.gdg_wave_bytes_per_sample(o.out_format)) // every port at the delivered rate (BatchSetDelivery, BatchSetDeliveryRatio)
	no := n + 3 + int(C.gdg_batch_blends(this.ctx)) // the blends in force (BatchSetBlends): one more port each, behind the metronome's
	outs := make([][]byte, no)
	if each == 0 {
		for i := range outs {
			outs[i] = []byte{}
		}
		return outs, nil
	}
	ptrs := (*[1 << 20]unsafe.Pointer)(C.calloc(C.size_t(no), C.size_t(unsafe.Sizeof(uintptr(0)))))
	if ptrs == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(ptrs))
	for i := 0; i < no; i++ {
		ptrs[i] = C.malloc(C.size_t(each))
		if ptrs[i] == nil {
			return nil, fmt.Errorf("gdg: out of memory (%d bytes per output)", each)
		}
		owned = append(owned, ptrs[i])
	}
	if e := this.err(C.gdg_batch_run(this.ctx, &arr[0], C.int(n), &o, (*unsafe.Pointer)(unsafe.Pointer(ptrs)))); e != nil {
		return nil, e
	}
	for i := range outs {
		outs[i] = goBytes(ptrs[i], each)
	}
	return outs, nil
}

// goBytes copies n bytes of C memory into a fresh slice.  C.GoBytes takes a C.int length and overflows from 2 GiB on
// (46 minutes of float64 at 96 kHz); this goes through a slice header over the C memory instead.
func goBytes(p unsafe.Pointer, n int) []byte {
	out := make([]byte, n)
	if n > 0 {
		copy(out, (*[1 << 40]byte)(p)[:n:n])
	}
	return out
}

func goFloats(p unsafe.Pointer, n int) []float64 {
	out := make([]float64, n)
	if n > 0 {
		copy(out, (*[1 << 37]float64)(p)[:n:n])
	}
	return out
}

// batchInputs builds the C array of gdg_batch_input; the file bytes live in C memory until release() is called.
func batchInputs(inputs []BatchInput) (arr *[1 << 20]C.gdg_batch_input, release func(), err error) {
	n := len(inputs)
	arr = (*[1 << 20]C.gdg_batch_input)(C.calloc(C.size_t(n), C.size_t(unsafe.Sizeof(C.gdg_batch_input{}))))
	if arr == nil {
		return nil, func() {}, fmt.Errorf("gdg: out of memory")
	}
	owned := []unsafe.Pointer{unsafe.Pointer(arr)}
	release = func() {
		for _, p := range owned {
			C.free(p)
		}
	}
	for i, in := range inputs {
		width := int(C.gdg_wave_bytes_per_sample(C.int(in.Format)))
		if len(in.Data) == 0 || width == 0 || in.Channels <= 0 {
			continue
		}
		p := C.CBytes(in.Data)
		if p == nil {
			release()
			return nil, func() {}, fmt.Errorf("gdg: out of memory")
		}
		owned = append(owned, p)
		arr[i].bytes = p
		arr[i].samples_per_channel = C.size_t(len(in.Data) / (width * in.Channels))
		arr[i].format = C.int(in.Format)
		arr[i].sample_rate = C.uint32_t(in.SampleRate)
		arr[i].channels = C.uint(in.Channels)
		arr[i].channel = C.uint(in.Channel)
	}
	return arr, release, nil
}

// BatchLength: samples of every output for these inputs (gdg_batch_length): the longest resampled input, rounded up to 8192.
func (this *Context) BatchLength(inputs []BatchInput, targetRate uint32) (int, error) {
	if len(inputs) == 0 {
		return 0, fmt.Errorf("gdg: no inputs")
	}
	arr, release, err := batchInputs(inputs)
	if err != nil {
		return 0, err
	}
	defer release()
	var samples C.size_t
	if e := this.err(C.gdg_batch_length(this.ctx, &arr[0], C.int(len(inputs)), C.uint32_t(targetRate), &samples)); e != nil {
		return 0, e
	}
	return int(samples), nil
}

// ShardResult: what one shard of a split job hands back (gdg_batch_run_shard).
type ShardResult struct {
	Outputs        [][]byte  // the shard's n encoded chain outputs
	Left, Right    []float64 // its PARTIAL master mix (no aux input, not clipped)
	MetronomeBytes []byte    // only on the shard that runs the metronome
	Metronome      []float64 // its float64 samples (the master's aux input when metrMasterOutput is set)
}

// BatchRunShard: the batch run of ONE shard of a job whose channels are split over several contexts / GPUs (contiguous channel
// blocks, gdg.Shards).  jobSamples = the longest BatchLength over all shards (every output of the job has that length,
// controller.go:3005-3045); exactly one shard passes runMetronome.  The master is finished once with FinishMaster.
func (this *Context) BatchRunShard(inputs []BatchInput, opt BatchOptions, jobSamples int, runMetronome bool) (*ShardResult, error) {
	n := len(inputs)
	if n == 0 {
		return nil, fmt.Errorf("gdg: no inputs")
	}
	arr, release, err := batchInputs(inputs)
	if err != nil {
		return nil, err
	}
	defer release()
	o := C.gdg_batch_options{target_rate: C.uint32_t(opt.TargetRate), out_format: C.int(opt.OutFormat),
		metronome_to_master: 0, run_meters: cbool(opt.RunMeters), tuner_enqueue: cbool(opt.TunerEnqueue)}
	width := int(C.gdg_wave_bytes_per_sample(o.out_format))
	res := &ShardResult{Outputs: make([][]byte, n)}
	if jobSamples == 0 || width == 0 {
		return res, nil
	}
	var owned []unsafe.Pointer
	defer func() {
		for _, p := range owned {
			C.free(p)
		}
	}()
	alloc := func(bytes int) unsafe.Pointer {
		p := C.malloc(C.size_t(bytes))
		if p != nil {
			owned = append(owned, p)
		}
		return p
	}
	ptrs := (*[1 << 20]unsafe.Pointer)(C.calloc(C.size_t(n), C.size_t(unsafe.Sizeof(uintptr(0)))))
	if ptrs == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	owned = append(owned, unsafe.Pointer(ptrs))
	for i := 0; i < n; i++ {
		if ptrs[i] = alloc(jobSamples * width); ptrs[i] == nil {
			return nil, fmt.Errorf("gdg: out of memory")
		}
	}
	var so C.gdg_batch_shard_out
	so.master_left = (*C.double)(alloc(jobSamples * 8))
	so.master_right = (*C.double)(alloc(jobSamples * 8))
	so.job_samples = C.size_t(jobSamples)
	if so.master_left == nil || so.master_right == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	if runMetronome {
		so.metronome_bytes = alloc(jobSamples * width)
		so.metronome = (*C.double)(alloc(jobSamples * 8))
		if so.metronome_bytes == nil || so.metronome == nil {
			return nil, fmt.Errorf("gdg: out of memory")
		}
	}
	if e := this.err(C.gdg_batch_run_shard(this.ctx, &arr[0], C.int(n), &o, (*unsafe.Pointer)(unsafe.Pointer(ptrs)), &so)); e != nil {
		return nil, e
	}
	for i := range res.Outputs {
		res.Outputs[i] = goBytes(ptrs[i], jobSamples*width)
	}
	res.Left = goFloats(unsafe.Pointer(so.master_left), jobSamples)
	res.Right = goFloats(unsafe.Pointer(so.master_right), jobSamples)
	if runMetronome {
		res.MetronomeBytes = goBytes(so.metronome_bytes, jobSamples*width)
		res.Metronome = goFloats(unsafe.Pointer(so.metronome), jobSamples)
	}
	return res, nil
}

// BatchStreamInput: one input file of the streamed batch run, described by its RIFF header alone: Frames is the FILE's total samples
// per channel (0 leaves the channel empty); the bytes come slice by slice.
type BatchStreamInput struct {
	Frames     uint64
	Format     int // gdg_wave_format
	SampleRate uint32
	Channels   int
	Channel    int
}

// BatchStreamOpen begins the job of BatchRun in slices of whole 8192-sample blocks (gdg_batch_stream_open): files of any length in
// bounded memory, the outputs byte for byte BatchRun's.  Returns the samples of every output.
func (this *Context) BatchStreamOpen(inputs []BatchStreamInput, opt BatchOptions) (uint64, error) {
	n := len(inputs)
	if n == 0 {
		return 0, fmt.Errorf("gdg: no inputs")
	}
	arr := (*[1 << 20]C.gdg_batch_input)(C.calloc(C.size_t(n), C.size_t(unsafe.Sizeof(C.gdg_batch_input{}))))
	if arr == nil {
		return 0, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(arr))
	for i, in := range inputs {
		if in.Frames == 0 {
			continue
		}
		arr[i].bytes = unsafe.Pointer(arr) // never read: only "not NULL"
		arr[i].samples_per_channel = C.size_t(in.Frames)
		arr[i].format = C.int(in.Format)
		arr[i].sample_rate = C.uint32_t(in.SampleRate)
		arr[i].channels = C.uint(in.Channels)
		arr[i].channel = C.uint(in.Channel)
	}
	o := C.gdg_batch_options{target_rate: C.uint32_t(opt.TargetRate), out_format: C.int(opt.OutFormat),
		metronome_to_master: cbool(opt.MetronomeToMaster), run_meters: cbool(opt.RunMeters), tuner_enqueue: cbool(opt.TunerEnqueue)}
	var samples C.size_t
	if e := this.err(C.gdg_batch_stream_open(this.ctx, &arr[0], C.int(n), &o, &samples)); e != nil {
		return 0, e
	}
	this.streamInputs = n
	this.streamWidth = int(C.gdg_wave_bytes_per_sample(o.out_format))
	this.streamDone = 0
	return uint64(samples), nil
}

// BatchStreamNeed: the source frames [first[i], first[i] + count[i]) of every input that the next slice of `blocks` blocks must bring.
func (this *Context) BatchStreamNeed(blocks int) (first []uint64, count []uint64, err error) {
	n := this.streamInputs
	if n == 0 {
		return nil, nil, fmt.Errorf("gdg: no streamed batch run is open")
	}
	buf := (*[1 << 20]C.size_t)(C.calloc(C.size_t(2*n), C.size_t(unsafe.Sizeof(C.size_t(0)))))
	if buf == nil {
		return nil, nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(buf))
	if e := this.err(C.gdg_batch_stream_need(this.ctx, C.int(blocks), &buf[0], &buf[n])); e != nil {
		return nil, nil, e
	}
	first, count = make([]uint64, n), make([]uint64, n)
	for i := 0; i < n; i++ {
		first[i], count[i] = uint64(buf[i]), uint64(buf[n+i])
	}
	return first, count, nil
}

// BatchStreamStep runs one slice: frames[i] holds the interleaved frames BatchStreamNeed asked for (nil where it asked for none);
// returns the slice's N + 3 output pieces of blocks * 8192 samples each.  The bytes live in C memory for the duration of the call.
func (this *Context) BatchStreamStep(blocks int, frames [][]byte) ([][]byte, error) {
	n := this.streamInputs
	if n == 0 || len(frames) != n {
		return nil, fmt.Errorf("gdg: %d inputs for a streamed batch run of %d", len(frames), n)
	}
	each := this.delivered(this.streamDone, blocks*8192) * this.streamWidth // every piece at the delivered rate (BatchSetDelivery, BatchSetDeliveryRatio)
	if blocks <= 0 || each <= 0 {
		return nil, fmt.Errorf("gdg: a slice of %d blocks", blocks)
	}
	var owned []unsafe.Pointer
	defer func() {
		for _, p := range owned {
			C.free(p)
		}
	}()
	no := n + 3 + int(C.gdg_batch_blends(this.ctx)) // the blends in force: they cannot change while the job is open
	ptrs := (*[1 << 20]unsafe.Pointer)(C.calloc(C.size_t(n+no), C.size_t(unsafe.Sizeof(uintptr(0)))))
	if ptrs == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(ptrs))
	for i, f := range frames {
		if len(f) == 0 {
			continue
		}
		ptrs[i] = C.CBytes(f)
		if ptrs[i] == nil {
			return nil, fmt.Errorf("gdg: out of memory (%d bytes of input %d)", len(f), i)
		}
		owned = append(owned, ptrs[i])
	}
	for i := n; i < n+no; i++ {
		ptrs[i] = C.malloc(C.size_t(each))
		if ptrs[i] == nil {
			return nil, fmt.Errorf("gdg: out of memory (%d bytes per output)", each)
		}
		owned = append(owned, ptrs[i])
	}
	if e := this.err(C.gdg_batch_stream_step(this.ctx, C.int(blocks), (*unsafe.Pointer)(unsafe.Pointer(&ptrs[0])), (*unsafe.Pointer)(unsafe.Pointer(&ptrs[n])))); e != nil {
		return nil, e
	}
	this.streamDone += blocks * 8192
	outs := make([][]byte, no)
	for i := range outs {
		outs[i] = goBytes(ptrs[n+i], each)
	}
	return outs, nil
}

// BatchStreamClose ends the streamed job, also before its last block (gdg_batch_stream_close); the context stays usable.
func (this *Context) BatchStreamClose() error {
	this.streamInputs = 0
	return this.err(C.gdg_batch_stream_close(this.ctx))
}

// BatchStreamCheckpoint writes the open streamed job (plain or a shard's) into one blob: its position, the channel state, the frames the
// resampler looks back at, meters, tuner rings and the metronome's counters (gdg_batch_stream_checkpoint).  Valid between any two
// slices, before the first and after the last; the context is not changed.  The blob carries a digest of its payload (StateVerify).
func (this *Context) BatchStreamCheckpoint() ([]byte, error) {
	var size C.size_t
	if err := this.err(C.gdg_batch_stream_checkpoint_size(this.ctx, &size)); err != nil {
		return nil, err
	}
	buf := make([]byte, int(size)+1)
	var written C.size_t
	if err := this.err(C.gdg_batch_stream_checkpoint(this.ctx, unsafe.Pointer(&buf[0]), size, &written)); err != nil {
		return nil, err
	}
	return buf[:int(written)], nil
}

// streamResume: BatchStreamResume and BatchStreamResumeShard.
func (this *Context) streamResume(inputs []BatchStreamInput, opt BatchOptions, shard bool, jobSamples uint64, runMetronome bool, blob []byte) (uint64, error) {
	n := len(inputs)
	if n == 0 {
		return 0, fmt.Errorf("gdg: no inputs")
	}
	if len(blob) == 0 {
		return 0, fmt.Errorf("gdg: an empty checkpoint")
	}
	arr := (*[1 << 20]C.gdg_batch_input)(C.calloc(C.size_t(n), C.size_t(unsafe.Sizeof(C.gdg_batch_input{}))))
	if arr == nil {
		return 0, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(arr))
	for i, in := range inputs {
		if in.Frames == 0 {
			continue
		}
		arr[i].bytes = unsafe.Pointer(arr) // never read: only "not NULL"
		arr[i].samples_per_channel = C.size_t(in.Frames)
		arr[i].format = C.int(in.Format)
		arr[i].sample_rate = C.uint32_t(in.SampleRate)
		arr[i].channels = C.uint(in.Channels)
		arr[i].channel = C.uint(in.Channel)
	}
	o := C.gdg_batch_options{target_rate: C.uint32_t(opt.TargetRate), out_format: C.int(opt.OutFormat),
		metronome_to_master: cbool(opt.MetronomeToMaster), run_meters: cbool(opt.RunMeters), tuner_enqueue: cbool(opt.TunerEnqueue)}
	var done C.size_t
	var rc C.int
	if shard {
		rc = C.gdg_batch_stream_resume_shard(this.ctx, &arr[0], C.int(n), &o, C.size_t(jobSamples), cbool(runMetronome), unsafe.Pointer(&blob[0]), C.size_t(len(blob)), &done)
	} else {
		rc = C.gdg_batch_stream_resume(this.ctx, &arr[0], C.int(n), &o, unsafe.Pointer(&blob[0]), C.size_t(len(blob)), &done)
	}
	if e := this.err(rc); e != nil {
		return 0, e
	}
	this.streamInputs = n
	this.streamWidth = int(C.gdg_wave_bytes_per_sample(o.out_format))
	this.streamDone = int(done)
	return uint64(done), nil
}

// BatchStreamResume takes the place of BatchStreamOpen on a context configured as for a fresh job (chains, parameters, taps,
// positions, metronome, meter ports): the job of the checkpoint, given again with inputs and opt, is open at the recorded position,
// which is returned (samples done).  All or nothing: a blob that is damaged or does not fit the job or the chains is an error, changes
// nothing and leaves no job open.
func (this *Context) BatchStreamResume(inputs []BatchStreamInput, opt BatchOptions, blob []byte) (uint64, error) {
	return this.streamResume(inputs, opt, false, 0, true, blob)
}

// BatchStreamResumeShard is BatchStreamResume for a job opened with BatchStreamOpenShard (same jobSamples and runMetronome).
func (this *Context) BatchStreamResumeShard(inputs []BatchStreamInput, opt BatchOptions, jobSamples uint64, runMetronome bool, blob []byte) (uint64, error) {
	return this.streamResume(inputs, opt, true, jobSamples, runMetronome, blob)
}

// StateVerify checks the digest of a checkpoint container on the device and writes nothing (gdg_state_verify).  The digest is for
// integrity only.  A bare SaveState blob has none and is an error.
func (this *Context) StateVerify(blob []byte) error {
	if len(blob) == 0 {
		return fmt.Errorf("gdg: an empty checkpoint")
	}
	return this.err(C.gdg_state_verify(this.ctx, unsafe.Pointer(&blob[0]), C.size_t(len(blob))))
}

// BatchStreamOpenShard begins the job of BatchRunShard in slices (gdg_batch_stream_open_shard): one shard of a job split over several
// contexts whose files are too long to hold.  jobSamples = the job's length (the longest BatchLength over all shards, 0 = this shard's
// own); runMetronome says once, for the whole job, whether this shard runs the metronome.  opt.MetronomeToMaster must be false: the aux
// input joins the master in FinishMasterSlice.  Returns the samples of every output.  BatchStreamNeed and BatchStreamClose serve the job.
func (this *Context) BatchStreamOpenShard(inputs []BatchStreamInput, opt BatchOptions, jobSamples uint64, runMetronome bool) (uint64, error) {
	n := len(inputs)
	if n == 0 {
		return 0, fmt.Errorf("gdg: no inputs")
	}
	arr := (*[1 << 20]C.gdg_batch_input)(C.calloc(C.size_t(n), C.size_t(unsafe.Sizeof(C.gdg_batch_input{}))))
	if arr == nil {
		return 0, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(arr))
	for i, in := range inputs {
		if in.Frames == 0 {
			continue
		}
		arr[i].bytes = unsafe.Pointer(arr) // never read: only "not NULL"
		arr[i].samples_per_channel = C.size_t(in.Frames)
		arr[i].format = C.int(in.Format)
		arr[i].sample_rate = C.uint32_t(in.SampleRate)
		arr[i].channels = C.uint(in.Channels)
		arr[i].channel = C.uint(in.Channel)
	}
	o := C.gdg_batch_options{target_rate: C.uint32_t(opt.TargetRate), out_format: C.int(opt.OutFormat),
		metronome_to_master: cbool(opt.MetronomeToMaster), run_meters: cbool(opt.RunMeters), tuner_enqueue: cbool(opt.TunerEnqueue)}
	var samples C.size_t
	if e := this.err(C.gdg_batch_stream_open_shard(this.ctx, &arr[0], C.int(n), &o, C.size_t(jobSamples), cbool(runMetronome), &samples)); e != nil {
		return 0, e
	}
	this.streamInputs = n
	this.streamWidth = int(C.gdg_wave_bytes_per_sample(o.out_format))
	return uint64(samples), nil
}

// BatchStreamStepShard runs one slice of a shard's job (gdg_batch_stream_step_shard): frames as for BatchStreamStep; the result holds the
// slice's n chain outputs, the shard's partial master mix of the slice and, with wantMetronome (only on a job opened with
// runMetronome), the slice's metronome track -- blocks * 8192 samples each.
func (this *Context) BatchStreamStepShard(blocks int, frames [][]byte, wantMetronome bool) (*ShardResult, error) {
	n := this.streamInputs
	if n == 0 || len(frames) != n {
		return nil, fmt.Errorf("gdg: %d inputs for a streamed batch run of %d", len(frames), n)
	}
	count := blocks * 8192
	each := count * this.streamWidth
	if blocks <= 0 || each <= 0 {
		return nil, fmt.Errorf("gdg: a slice of %d blocks", blocks)
	}
	var owned []unsafe.Pointer
	defer func() {
		for _, p := range owned {
			C.free(p)
		}
	}()
	alloc := func(bytes int) unsafe.Pointer {
		p := C.malloc(C.size_t(bytes))
		if p != nil {
			owned = append(owned, p)
		}
		return p
	}
	ptrs := (*[1 << 20]unsafe.Pointer)(C.calloc(C.size_t(2*n), C.size_t(unsafe.Sizeof(uintptr(0)))))
	if ptrs == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(ptrs))
	for i, f := range frames {
		if len(f) == 0 {
			continue
		}
		ptrs[i] = C.CBytes(f)
		if ptrs[i] == nil {
			return nil, fmt.Errorf("gdg: out of memory (%d bytes of input %d)", len(f), i)
		}
		owned = append(owned, ptrs[i])
	}
	for i := n; i < 2*n; i++ {
		if ptrs[i] = alloc(each); ptrs[i] == nil {
			return nil, fmt.Errorf("gdg: out of memory (%d bytes per output)", each)
		}
	}
	var so C.gdg_batch_shard_out
	so.master_left = (*C.double)(alloc(count * 8))
	so.master_right = (*C.double)(alloc(count * 8))
	if so.master_left == nil || so.master_right == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	if wantMetronome {
		so.metronome_bytes = alloc(each)
		so.metronome = (*C.double)(alloc(count * 8))
		if so.metronome_bytes == nil || so.metronome == nil {
			return nil, fmt.Errorf("gdg: out of memory")
		}
	}
	if e := this.err(C.gdg_batch_stream_step_shard(this.ctx, C.int(blocks), (*unsafe.Pointer)(unsafe.Pointer(&ptrs[0])), (*unsafe.Pointer)(unsafe.Pointer(&ptrs[n])), &so)); e != nil {
		return nil, e
	}
	res := &ShardResult{Outputs: make([][]byte, n)}
	for i := range res.Outputs {
		res.Outputs[i] = goBytes(ptrs[n+i], each)
	}
	res.Left = goFloats(unsafe.Pointer(so.master_left), count)
	res.Right = goFloats(unsafe.Pointer(so.master_right), count)
	if wantMetronome {
		res.MetronomeBytes = goBytes(so.metronome_bytes, each)
		res.Metronome = goFloats(unsafe.Pointer(so.metronome), count)
	}
	return res, nil
}

// BatchRelease returns the device buffers of the last batch run to the context's arena (gdg_batch_release); the next run re-makes them.
func (this *Context) BatchRelease() error { return this.err(C.gdg_batch_release(this.ctx)) }

// Synchronize waits for everything the context has launched (gdg_ctx_synchronize); the host-buffer calls above already do.
func (this *Context) Synchronize() error { return this.err(C.gdg_ctx_synchronize(this.ctx)) }

// Version of the library behind the binding (gdg_version).
func Version() string { return C.GoString(C.gdg_version()) }

// FinishMaster: master = ((p_0 + p_1) + ... + p_{G-1}) + aux per side, summed and encoded on this context's device
// (gdg_batch_finish_master; spatializer/spatializer.go:300-310, controller/controller.go:3123-3219).  aux == nil: no aux input.
func (this *Context) FinishMaster(outFormat int, shards []*ShardResult, aux []float64, sampleRate uint32, runMeters bool) (left []byte, right []byte, err error) {
	return this.finishMaster(false, outFormat, shards, aux, sampleRate, runMeters)
}

// FinishMasterSlice: FinishMaster for one slice of a streamed sharded job (gdg_batch_finish_master_slice): shards = every shard's
// BatchStreamStepShard result of the slice, in shard order; the same bytes, made for the job's critical path (one upload, one kernel
// and one download per piece).  A context runs one call at a time: a caller who wants the finish beside shard 0's next slice gives it
// a context of its own.
func (this *Context) FinishMasterSlice(outFormat int, shards []*ShardResult, aux []float64, sampleRate uint32, runMeters bool) (left []byte, right []byte, err error) {
	return this.finishMaster(true, outFormat, shards, aux, sampleRate, runMeters)
}

func (this *Context) finishMaster(slice bool, outFormat int, shards []*ShardResult, aux []float64, sampleRate uint32, runMeters bool) (left []byte, right []byte, err error) {
	g := len(shards)
	if g == 0 {
		return nil, nil, fmt.Errorf("gdg: no shards")
	}
	samples := len(shards[0].Left)
	width := int(C.gdg_wave_bytes_per_sample(C.int(outFormat)))
	if samples == 0 || width == 0 {
		return []byte{}, []byte{}, nil
	}
	var owned []unsafe.Pointer
	defer func() {
		for _, p := range owned {
			C.free(p)
		}
	}()
	cFloats := func(v []float64) *C.double {
		p := C.malloc(C.size_t(len(v) * 8))
		if p == nil {
			return nil
		}
		owned = append(owned, p)
		copy((*[1 << 37]float64)(p)[:len(v):len(v)], v)
		return (*C.double)(p)
	}
	lp := (*[1 << 20]*C.double)(C.calloc(C.size_t(2*g), C.size_t(unsafe.Sizeof(uintptr(0)))))
	if lp == nil {
		return nil, nil, fmt.Errorf("gdg: out of memory")
	}
	owned = append(owned, unsafe.Pointer(lp))
	for i, s := range shards {
		if len(s.Left) != samples || len(s.Right) != samples {
			return nil, nil, fmt.Errorf("gdg: shard %d has %d samples, shard 0 has %d", i, len(s.Left), samples)
		}
		lp[i], lp[g+i] = cFloats(s.Left), cFloats(s.Right)
		if lp[i] == nil || lp[g+i] == nil {
			return nil, nil, fmt.Errorf("gdg: out of memory")
		}
	}
	var cAux *C.double
	if aux != nil {
		if len(aux) != samples {
			return nil, nil, fmt.Errorf("gdg: the aux input has %d samples, the job %d", len(aux), samples)
		}
		if cAux = cFloats(aux); cAux == nil {
			return nil, nil, fmt.Errorf("gdg: out of memory")
		}
	}
	lb, rb := C.malloc(C.size_t(samples*width)), C.malloc(C.size_t(samples*width))
	if lb == nil || rb == nil {
		C.free(lb)
		C.free(rb)
		return nil, nil, fmt.Errorf("gdg: out of memory")
	}
	owned = append(owned, lb, rb)
	if slice {
		if e := this.err(C.gdg_batch_finish_master_slice(this.ctx, C.int(outFormat), &lp[0], &lp[g], C.int(g), cAux, C.size_t(samples), C.uint32_t(sampleRate),
			cbool(runMeters), lb, rb)); e != nil {
			return nil, nil, e
		}
	} else if e := this.err(C.gdg_batch_finish_master(this.ctx, C.int(outFormat), &lp[0], &lp[g], C.int(g), cAux, C.size_t(samples), C.uint32_t(sampleRate),
		cbool(runMeters), lb, rb)); e != nil {
		return nil, nil, e
	}
	return goBytes(lb, samples*width), goBytes(rb, samples*width), nil
}

// BlockStats is one record of the render report (gdg_block_stats): what one block of one output port held just before the encoder
// read it.  Peak: max |x| over the finite samples; SumSq: the sum of their squares, added in an order that depends on the block's
// length alone; PeakIndex: the first index with |x| == Peak; Clipped: |x| > 1 (the samples the encoder's clamp changes); FullScale:
// |x| >= 1; Nonfinite: NaN and +-Inf, counted and left out of the rest.
type BlockStats struct {
	Peak      float64
	SumSq     float64
	PeakIndex uint32
	Clipped   uint32
	FullScale uint32
	Nonfinite uint32
}

func goBlockStats(p unsafe.Pointer, rows int, blocks int) [][]BlockStats {
	out := make([][]BlockStats, rows)
	if rows*blocks == 0 {
		for r := range out {
			out[r] = []BlockStats{}
		}
		return out
	}
	recs := (*[1 << 26]C.gdg_block_stats)(p)[: rows*blocks : rows*blocks]
	for r := range out {
		out[r] = make([]BlockStats, blocks)
		for b := range out[r] {
			c := recs[r*blocks+b]
			out[r][b] = BlockStats{float64(c.peak), float64(c.sum_sq), uint32(c.peak_index), uint32(c.clipped), uint32(c.full_scale), uint32(c.nonfinite)}
		}
	}
	return out
}

// BlockStatsRows: the records of equally long host rows cut into blocks of `block` samples, the last one of a row possibly short
// (gdg_block_stats_rows); result[row][block].
func (this *Context) BlockStatsRows(rows [][]float64, block int) ([][]BlockStats, error) {
	n := len(rows)
	if n == 0 {
		return [][]BlockStats{}, nil
	}
	if block < 1 {
		return nil, fmt.Errorf("gdg: a block has at least one sample")
	}
	samples := len(rows[0])
	blocks := (samples + block - 1) / block
	if samples == 0 {
		return goBlockStats(nil, n, 0), nil
	}
	var owned []unsafe.Pointer
	defer func() {
		for _, p := range owned {
			C.free(p)
		}
	}()
	rp := (*[1 << 20]*C.double)(C.calloc(C.size_t(n), C.size_t(unsafe.Sizeof(uintptr(0)))))
	if rp == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	owned = append(owned, unsafe.Pointer(rp))
	for i, r := range rows {
		if len(r) != samples {
			return nil, fmt.Errorf("gdg: row %d has %d samples, row 0 has %d", i, len(r), samples)
		}
		p := C.malloc(C.size_t(samples * 8))
		if p == nil {
			return nil, fmt.Errorf("gdg: out of memory")
		}
		owned = append(owned, p)
		copy((*[1 << 37]float64)(p)[:samples:samples], r)
		rp[i] = (*C.double)(p)
	}
	rec := C.calloc(C.size_t(n*blocks), 32)
	if rec == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	owned = append(owned, rec)
	if e := this.err(C.gdg_block_stats_rows(this.ctx, &rp[0], C.int(n), C.size_t(samples), C.int(block), (*C.gdg_block_stats)(rec))); e != nil {
		return nil, e
	}
	return goBlockStats(rec, n, blocks), nil
}

// BlockStatsRowsDevice: the same on device memory, enqueued on the context's stream (gdg_block_stats_rows_device): row r at
// dRows + r*rowStride float64 (any 8-byte alignment, rowStride >= samples), the records into dRecords[nRows][ceil(samples/block)].
func (this *Context) BlockStatsRowsDevice(dRows unsafe.Pointer, rowStride int, nRows int, samples int, block int, dRecords unsafe.Pointer) error {
	return this.err(C.gdg_block_stats_rows_device(this.ctx, (*C.double)(dRows), C.size_t(rowStride), C.int(nRows), C.size_t(samples), C.int(block),
		(*C.gdg_block_stats)(dRecords)))
}

// BatchReportEnable: from the next batch call on, every batch call of the context keeps the records of what it rendered, per output
// port and block of 8192 samples (gdg_batch_report_enable).  Configuration, like the window: a checkpoint does not carry it -- set it
// again on the target of a resume.
func (this *Context) BatchReportEnable(enable bool) error {
	return this.err(C.gdg_batch_report_enable(this.ctx, cbool(enable)))
}

// BatchReport: the records of the last completed batch call, result[port][block] (gdg_batch_report).  BatchRun and BatchStreamStep
// report the N chain outputs, master left, master right and the metronome; a shard's calls its n chain outputs and the metronome;
// FinishMaster and FinishMasterSlice master left and right.  An error when the call ran without the report enabled.
func (this *Context) BatchReport() ([][]BlockStats, error) {
	var ports C.int
	var blocks C.size_t
	if e := this.err(C.gdg_batch_report(this.ctx, nil, 0, &ports, &blocks)); e != nil {
		return nil, e
	}
	n := int(ports) * int(blocks)
	if n == 0 {
		return goBlockStats(nil, int(ports), int(blocks)), nil
	}
	rec := C.calloc(C.size_t(n), 32)
	if rec == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(rec)
	if e := this.err(C.gdg_batch_report(this.ctx, (*C.gdg_block_stats)(rec), C.size_t(n), &ports, &blocks)); e != nil {
		return nil, e
	}
	return goBlockStats(rec, int(ports), int(blocks)), nil
}

// cEdges: an edge list of the band spectrum in C memory (the caller frees it); the library validates it.
func cEdges(edges []float64) (unsafe.Pointer, error) {
	n := len(edges)
	if n == 0 {
		return nil, fmt.Errorf("gdg: no edges")
	}
	p := C.malloc(C.size_t(n * 8))
	if p == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	copy((*[1 << 20]float64)(p)[:n:n], edges)
	return p, nil
}

// goSpectrum: [rows][blocks][bands] from the library's row-major float64 values.
func goSpectrum(p unsafe.Pointer, rows int, blocks int, bands int) [][][]float64 {
	out := make([][][]float64, rows)
	for r := 0; r < rows; r++ {
		out[r] = make([][]float64, blocks)
		for b := 0; b < blocks; b++ {
			out[r][b] = make([]float64, bands)
			if p != nil && bands > 0 {
				at := (r*blocks + b) * bands
				copy(out[r][b], (*[1 << 37]float64)(p)[at:at+bands:at+bands])
			}
		}
	}
	return out
}

// BlockSpectrumRows: the band powers of equally long host rows, per block of 8192 samples (the last one of a row possibly short:
// zero-padded) and per band between the edges in Hz (gdg_block_spectrum_rows): periodic Hann window, 8192-point transform, bin powers
// summed from ceil(edge*8192/rate) on; result[row][block][band].  2 to 33 edges, finite, >= 0, strictly ascending.
func (this *Context) BlockSpectrumRows(rows [][]float64, sampleRate uint32, edges []float64) ([][][]float64, error) {
	n := len(rows)
	if n == 0 {
		return [][][]float64{}, nil
	}
	samples := len(rows[0])
	blocks := (samples + 8191) / 8192
	var owned []unsafe.Pointer
	defer func() {
		for _, p := range owned {
			C.free(p)
		}
	}()
	ep, e := cEdges(edges)
	if e != nil {
		return nil, e
	}
	owned = append(owned, ep)
	bands := len(edges) - 1
	rp := (*[1 << 20]*C.double)(C.calloc(C.size_t(n), C.size_t(unsafe.Sizeof(uintptr(0)))))
	if rp == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	owned = append(owned, unsafe.Pointer(rp))
	for i, r := range rows {
		if len(r) != samples {
			return nil, fmt.Errorf("gdg: row %d has %d samples, row 0 has %d", i, len(r), samples)
		}
		p := C.malloc(C.size_t(samples*8 + 8))
		if p == nil {
			return nil, fmt.Errorf("gdg: out of memory")
		}
		owned = append(owned, p)
		copy((*[1 << 37]float64)(p)[:samples:samples], r)
		rp[i] = (*C.double)(p)
	}
	out := C.calloc(C.size_t(n*blocks*bands+1), 8)
	if out == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	owned = append(owned, out)
	if e := this.err(C.gdg_block_spectrum_rows(this.ctx, &rp[0], C.int(n), C.size_t(samples), C.uint32_t(sampleRate), (*C.double)(ep), C.int(len(edges)),
		(*C.double)(out))); e != nil {
		return nil, e
	}
	return goSpectrum(out, n, blocks, bands), nil
}

// BlockSpectrumRowsDevice: the same on device memory, enqueued on the context's stream (gdg_block_spectrum_rows_device): row r at
// dRows + r*rowStride float64 (any 8-byte alignment, rowStride >= samples), the bands into dBands[nRows][ceil(samples/8192)][len(edges)-1].
func (this *Context) BlockSpectrumRowsDevice(dRows unsafe.Pointer, rowStride int, nRows int, samples int, sampleRate uint32, edges []float64, dBands unsafe.Pointer) error {
	ep, e := cEdges(edges)
	if e != nil {
		return e
	}
	defer C.free(ep)
	return this.err(C.gdg_block_spectrum_rows_device(this.ctx, (*C.double)(dRows), C.size_t(rowStride), C.int(nRows), C.size_t(samples), C.uint32_t(sampleRate),
		(*C.double)(ep), C.int(len(edges)), (*C.double)(dBands)))
}

// BatchSpectrumEnable: from the next batch call on, every batch call of the context keeps the band powers of what it rendered, per output
// port, block of 8192 samples and band between the edges in Hz, at the job's rate (gdg_batch_spectrum_enable); nil or an empty slice
// switches it off.  Configuration, like BatchReportEnable: a checkpoint does not carry it -- set it again on the target of a resume --
// and an error while a streamed job is open.
func (this *Context) BatchSpectrumEnable(edges []float64) error {
	if len(edges) == 0 {
		return this.err(C.gdg_batch_spectrum_enable(this.ctx, nil, 0))
	}
	ep, e := cEdges(edges)
	if e != nil {
		return e
	}
	defer C.free(ep)
	return this.err(C.gdg_batch_spectrum_enable(this.ctx, (*C.double)(ep), C.int(len(edges))))
}

// BatchSpectrum: the band powers of the last completed batch call, result[port][block][band] (gdg_batch_spectrum); the ports and their
// order are BatchReport's.  An error when the call ran without the spectrum enabled.
func (this *Context) BatchSpectrum() ([][][]float64, error) {
	var ports C.int
	var blocks C.size_t
	var bands C.int
	if e := this.err(C.gdg_batch_spectrum(this.ctx, nil, 0, &ports, &blocks, &bands)); e != nil {
		return nil, e
	}
	n := int(ports) * int(blocks) * int(bands)
	if n == 0 {
		return goSpectrum(nil, int(ports), int(blocks), int(bands)), nil
	}
	val := C.calloc(C.size_t(n), 8)
	if val == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(val)
	if e := this.err(C.gdg_batch_spectrum(this.ctx, (*C.double)(val), C.size_t(n), &ports, &blocks, &bands)); e != nil {
		return nil, e
	}
	return goSpectrum(val, int(ports), int(blocks), int(bands)), nil
}

// BlockAlign: one record of the alignment report (gdg_block_align): lag and polarity of a block of 8192 samples of one row against the
// same block of its reference row.  Corr = r[Lag], signed (negative: opposite polarity); Corr0 = r[0]; Corr / sqrt(RefSq * SqAtLag) is the
// normalised coefficient.  A positive Lag: the row arrives later than its reference.
type BlockAlign struct {
	Corr    float64
	Corr0   float64
	RefSq   float64
	SqAtLag float64
	Lag     int32
}

func goBlockAlign(p unsafe.Pointer, rows int, blocks int) [][]BlockAlign {
	out := make([][]BlockAlign, rows)
	if rows*blocks == 0 {
		for r := range out {
			out[r] = []BlockAlign{}
		}
		return out
	}
	recs := (*[1 << 25]C.gdg_block_align)(p)[: rows*blocks : rows*blocks]
	for r := range out {
		out[r] = make([]BlockAlign, blocks)
		for b := range out[r] {
			c := recs[r*blocks+b]
			out[r][b] = BlockAlign{float64(c.corr), float64(c.corr0), float64(c.ref_sq), float64(c.sq_at_lag), int32(c.lag)}
		}
	}
	return out
}

// cRefs: a reference list of the alignment report in C memory (the caller frees it); the library validates it.
func cRefs(ref []int) (unsafe.Pointer, error) {
	n := len(ref)
	if n == 0 {
		return nil, fmt.Errorf("gdg: no references")
	}
	p := C.malloc(C.size_t(n * 4))
	if p == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	dst := (*[1 << 28]C.int)(p)[:n:n]
	for i, v := range ref {
		dst[i] = C.int(v)
	}
	return p, nil
}

// BlockAlignRows: the alignment records of equally long host rows, per block of 8192 samples (the last one of a row possibly short:
// zero-padded): row r against row ref[r], -1 for a row that is not measured (gdg_block_align_rows); 1 <= maxLag <= 2048;
// result[row][block].
func (this *Context) BlockAlignRows(rows [][]float64, ref []int, maxLag int) ([][]BlockAlign, error) {
	n := len(rows)
	if n == 0 {
		return [][]BlockAlign{}, nil
	}
	if len(ref) != n {
		return nil, fmt.Errorf("gdg: %d references for %d rows", len(ref), n)
	}
	samples := len(rows[0])
	blocks := (samples + 8191) / 8192
	var owned []unsafe.Pointer
	defer func() {
		for _, p := range owned {
			C.free(p)
		}
	}()
	fp, e := cRefs(ref)
	if e != nil {
		return nil, e
	}
	owned = append(owned, fp)
	rp := (*[1 << 20]*C.double)(C.calloc(C.size_t(n), C.size_t(unsafe.Sizeof(uintptr(0)))))
	if rp == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	owned = append(owned, unsafe.Pointer(rp))
	for i, r := range rows {
		if len(r) != samples {
			return nil, fmt.Errorf("gdg: row %d has %d samples, row 0 has %d", i, len(r), samples)
		}
		p := C.malloc(C.size_t(samples*8 + 8))
		if p == nil {
			return nil, fmt.Errorf("gdg: out of memory")
		}
		owned = append(owned, p)
		copy((*[1 << 37]float64)(p)[:samples:samples], r)
		rp[i] = (*C.double)(p)
	}
	out := C.calloc(C.size_t(n*blocks+1), 40)
	if out == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	owned = append(owned, out)
	if e := this.err(C.gdg_block_align_rows(this.ctx, &rp[0], C.int(n), C.size_t(samples), (*C.int)(fp), C.int(maxLag), (*C.gdg_block_align)(out))); e != nil {
		return nil, e
	}
	return goBlockAlign(out, n, blocks), nil
}

// BlockAlignRowsDevice: the same on device memory, enqueued on the context's stream (gdg_block_align_rows_device): row r at
// dRows + r*rowStride float64 (any 8-byte alignment, rowStride >= samples), the records into dRecords[len(ref)][ceil(samples/8192)].
func (this *Context) BlockAlignRowsDevice(dRows unsafe.Pointer, rowStride int, samples int, ref []int, maxLag int, dRecords unsafe.Pointer) error {
	fp, e := cRefs(ref)
	if e != nil {
		return e
	}
	defer C.free(fp)
	return this.err(C.gdg_block_align_rows_device(this.ctx, (*C.double)(dRows), C.size_t(rowStride), C.int(len(ref)), C.size_t(samples), (*C.int)(fp), C.int(maxLag),
		(*C.gdg_block_align)(dRecords)))
}

// BatchAlignEnable: from the next batch call on, every batch call of the context keeps the alignment records of what it rendered: port p
// against port ref[p], -1 for a port that is not measured, one entry per port of the calls to come (gdg_batch_align_enable); nil or an
// empty slice switches it off.  Configuration, like BatchSpectrumEnable: a checkpoint does not carry it -- set it again on the target of
// a resume -- and an error while a streamed job is open.
func (this *Context) BatchAlignEnable(ref []int, maxLag int) error {
	if len(ref) == 0 {
		return this.err(C.gdg_batch_align_enable(this.ctx, nil, 0, 0))
	}
	fp, e := cRefs(ref)
	if e != nil {
		return e
	}
	defer C.free(fp)
	return this.err(C.gdg_batch_align_enable(this.ctx, (*C.int)(fp), C.int(len(ref)), C.int(maxLag)))
}

// BatchAlign: the alignment records of the last completed batch call, result[port][block] (gdg_batch_align); the ports and their order
// are BatchReport's.  An error when the call ran without them, or was a master finish.
func (this *Context) BatchAlign() ([][]BlockAlign, error) {
	var ports C.int
	var blocks C.size_t
	if e := this.err(C.gdg_batch_align(this.ctx, nil, 0, &ports, &blocks)); e != nil {
		return nil, e
	}
	n := int(ports) * int(blocks)
	if n == 0 {
		return goBlockAlign(nil, int(ports), int(blocks)), nil
	}
	rec := C.calloc(C.size_t(n), 40)
	if rec == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(rec)
	if e := this.err(C.gdg_batch_align(this.ctx, (*C.gdg_block_align)(rec), C.size_t(n), &ports, &blocks)); e != nil {
		return nil, e
	}
	return goBlockAlign(rec, int(ports), int(blocks)), nil
}

// BlockTruePeak: one true-peak record (gdg_block_true_peak): the largest magnitude of a block of 8192 samples 4x oversampled -- its samples
// and the three points a 24-tap windowed-sinc interpolator puts between two of them.  Position = 4*n + phase (phase 0: a sample) of the
// first point that attains it; Overs counts the interpolated points above 1.
type BlockTruePeak struct {
	TruePeak float64
	Position uint32
	Overs    uint32
}

func goBlockTruePeak(p unsafe.Pointer, rows int, blocks int) [][]BlockTruePeak {
	out := make([][]BlockTruePeak, rows)
	if rows*blocks == 0 {
		for r := range out {
			out[r] = []BlockTruePeak{}
		}
		return out
	}
	recs := (*[1 << 26]C.gdg_block_true_peak)(p)[: rows*blocks : rows*blocks]
	for r := range out {
		out[r] = make([]BlockTruePeak, blocks)
		for b := range out[r] {
			c := recs[r*blocks+b]
			out[r][b] = BlockTruePeak{float64(c.true_peak), uint32(c.position), uint32(c.overs)}
		}
	}
	return out
}

// TruePeakTaps: the library's interpolation taps (gdg_true_peak_taps): result[phase-1][j+11] for phase 1, 2, 3 and j = -11 .. 12.
// No context and no device are needed.
func TruePeakTaps() ([3][24]float64, error) {
	var out [3][24]float64
	p := C.malloc(C.size_t(72 * 8))
	if p == nil {
		return out, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(p)
	if rc := C.gdg_true_peak_taps((*C.double)(p), C.int(72)); rc != 0 {
		return out, fmt.Errorf("gdg: gdg_true_peak_taps: %d", int(rc))
	}
	flat := (*[72]float64)(p)
	for i := 0; i < 72; i++ {
		out[i/24][i%24] = flat[i]
	}
	return out, nil
}

// BlockTruePeakRows: the true-peak records of equally long host rows, per block of 8192 samples (the last one of a row possibly short)
// (gdg_block_true_peak_rows); result[row][block].
func (this *Context) BlockTruePeakRows(rows [][]float64) ([][]BlockTruePeak, error) {
	n := len(rows)
	if n == 0 {
		return [][]BlockTruePeak{}, nil
	}
	samples := len(rows[0])
	blocks := (samples + 8191) / 8192
	var owned []unsafe.Pointer
	defer func() {
		for _, p := range owned {
			C.free(p)
		}
	}()
	rp := (*[1 << 20]*C.double)(C.calloc(C.size_t(n), C.size_t(unsafe.Sizeof(uintptr(0)))))
	if rp == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	owned = append(owned, unsafe.Pointer(rp))
	for i, r := range rows {
		if len(r) != samples {
			return nil, fmt.Errorf("gdg: row %d has %d samples, row 0 has %d", i, len(r), samples)
		}
		p := C.malloc(C.size_t(samples*8 + 8))
		if p == nil {
			return nil, fmt.Errorf("gdg: out of memory")
		}
		owned = append(owned, p)
		copy((*[1 << 37]float64)(p)[:samples:samples], r)
		rp[i] = (*C.double)(p)
	}
	out := C.calloc(C.size_t(n*blocks+1), 16)
	if out == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	owned = append(owned, out)
	if e := this.err(C.gdg_block_true_peak_rows(this.ctx, &rp[0], C.int(n), C.size_t(samples), (*C.gdg_block_true_peak)(out))); e != nil {
		return nil, e
	}
	return goBlockTruePeak(out, n, blocks), nil
}

// BlockTruePeakRowsDevice: the same on device memory, enqueued on the context's stream (gdg_block_true_peak_rows_device): row r at
// dRows + r*rowStride float64 (any 8-byte alignment, rowStride >= samples), the records into dRecords[nRows][ceil(samples/8192)].
func (this *Context) BlockTruePeakRowsDevice(dRows unsafe.Pointer, rowStride int, nRows int, samples int, dRecords unsafe.Pointer) error {
	return this.err(C.gdg_block_true_peak_rows_device(this.ctx, (*C.double)(dRows), C.size_t(rowStride), C.int(nRows), C.size_t(samples),
		(*C.gdg_block_true_peak)(dRecords)))
}

// BatchTruePeakEnable: from the next batch call on, every batch call of the context keeps the true-peak records of what it rendered
// (gdg_batch_true_peak_enable); off by default.  Configuration, like BatchReportEnable: a checkpoint does not carry it -- set it again
// on the target of a resume -- and an error while a streamed job is open.
func (this *Context) BatchTruePeakEnable(enable bool) error {
	v := C.int(0)
	if enable {
		v = 1
	}
	return this.err(C.gdg_batch_true_peak_enable(this.ctx, v))
}

// BatchTruePeak: the true-peak records of the last completed batch call, result[port][block] (gdg_batch_true_peak); the ports and their
// order are BatchReport's, the two finish calls included.  An error when the call ran without them.
func (this *Context) BatchTruePeak() ([][]BlockTruePeak, error) {
	var ports C.int
	var blocks C.size_t
	if e := this.err(C.gdg_batch_true_peak(this.ctx, nil, 0, &ports, &blocks)); e != nil {
		return nil, e
	}
	n := int(ports) * int(blocks)
	if n == 0 {
		return goBlockTruePeak(nil, int(ports), int(blocks)), nil
	}
	rec := C.calloc(C.size_t(n), 16)
	if rec == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(rec)
	if e := this.err(C.gdg_batch_true_peak(this.ctx, (*C.gdg_block_true_peak)(rec), C.size_t(n), &ports, &blocks)); e != nil {
		return nil, e
	}
	return goBlockTruePeak(rec, int(ports), int(blocks)), nil
}

// BatchSetSources: the source map of the next batch calls (gdg_batch_set_sources): source[c] is the channel whose input entry channel c
// reads -- c itself for a channel that reads its own, a root; any other entry makes c a reader, and its source must be a root.  One entry
// per channel; nil or an empty slice clears the map.  A shared input is uploaded, decoded and resampled once and stored to every row
// that reads it; the outputs are those of the job with the entry copied.  Configuration, like the window: no blob carries it, and a job
// with a reader cannot be checkpointed yet.
func (this *Context) BatchSetSources(source []int) error {
	n := len(source)
	if n == 0 {
		return this.err(C.gdg_batch_set_sources(this.ctx, nil, 0))
	}
	p := (*[1 << 28]C.int)(C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(C.int(0)))))
	if p == nil {
		return fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(p))
	for i, v := range source {
		p[i] = C.int(v)
	}
	return this.err(C.gdg_batch_set_sources(this.ctx, &p[0], C.int(n)))
}

// Ports of the job-wide outputs under dither (gdg_batch_set_dither): a shard need not know the job's channel count.
const (
	DitherPortMasterLeft  = 0xfffffffd
	DitherPortMasterRight = 0xfffffffe
	DitherPortMetronome   = 0xffffffff
)

// BatchSetDither: the dither of the LPCM outputs of the next batch calls (gdg_batch_set_dither).  mode 0 is off, 1 is TPDF with
// rounding; the noise of a sample depends on (seed, port, sample index) alone, so a file has the same bytes however the job is cut;
// portBase is the job-wide index of this context's first channel (0 for an unsharded job).  Configuration, like the window: a
// checkpoint does not carry it -- set it again on the target of a resume.  Resets the master cursor to 0.
func (this *Context) BatchSetDither(mode int, seed uint64, portBase uint32) error {
	return this.err(C.gdg_batch_set_dither(this.ctx, C.int(mode), C.uint64_t(seed), C.uint32_t(portBase)))
}

// BatchDitherSeek: the sample index the next FinishMasterSlice starts at (gdg_batch_dither_seek); a finished slice moves it on by its
// samples.  A caller that resumes a sharded job from a checkpoint seeks to the samples done.
func (this *Context) BatchDitherSeek(sampleIndex uint64) error {
	return this.err(C.gdg_batch_dither_seek(this.ctx, C.uint64_t(sampleIndex)))
}

// WaveEncodeDither: one mono row through the dithered encoder (gdg_wave_encode_dither); sample i has index firstIndex + i.  mode 0, or an
// IEEE format, gives WaveEncode's bytes.
func (this *Context) WaveEncodeDither(format int, samples []float64, mode int, seed uint64, port uint32, firstIndex uint64) ([]byte, error) {
	width := int(C.gdg_wave_bytes_per_sample(C.int(format)))
	if width == 0 {
		return nil, fmt.Errorf("gdg: unknown sample format %d", format)
	}
	data := make([]byte, len(samples)*width)
	if len(samples) == 0 {
		return data, nil
	}
	rc := C.gdg_wave_encode_dither(this.ctx, C.int(format), (*C.double)(unsafe.Pointer(&samples[0])), C.size_t(len(samples)), C.int(mode), C.uint64_t(seed), C.uint32_t(port), C.uint64_t(firstIndex), unsafe.Pointer(&data[0]))
	return data, this.err(rc)
}

// BatchSetTrim: the output trim of the next batch calls (gdg_batch_set_trim): a gain per output port in front of the encoders.  chainGain
// has one entry per channel of this context (a shard passes its own channels'; nil or empty: every chain gain 1); masterLeft, masterRight
// and metronome are the gains of the job-wide ports.  y = x * g, rounded once, then the encoder as ever; a negative gain inverts the
// polarity.  Records, meters, float64 partials and the channel state stay as rendered.  All gains 1: off.  Configuration, like
// BatchSetDither: a checkpoint does not carry it -- set it again on the target of a resume -- and an error while a streamed job is open.
func (this *Context) BatchSetTrim(chainGain []float64, masterLeft float64, masterRight float64, metronome float64) error {
	n := len(chainGain)
	if n == 0 {
		return this.err(C.gdg_batch_set_trim(this.ctx, nil, 0, C.double(masterLeft), C.double(masterRight), C.double(metronome)))
	}
	p := (*[1 << 28]C.double)(C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(C.double(0)))))
	if p == nil {
		return fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(p))
	for i, v := range chainGain {
		p[i] = C.double(v)
	}
	return this.err(C.gdg_batch_set_trim(this.ctx, &p[0], C.int(n), C.double(masterLeft), C.double(masterRight), C.double(metronome)))
}

// DeliverHistory: the session samples a delivered row keeps from call to call (GDG_DELIVER_HISTORY of the C header).
const DeliverHistory = 154

// BatchSetDelivery: from the next batch call on BatchRun and BatchStreamStep write every port -- chain outputs, master left and right,
// metronome, blends -- at 1 / factor of the session rate (gdg_batch_set_delivery): factor 1 (off), 2 or 4.  The reference's decimator
// (oversampling.Decimate: the anti-aliasing FIR of 77 or 155 taps, every factor-th sample, times ATTENUATION_HALF_DECIBEL) on the finished
// float64 rows; an output has samples / factor samples and lags the render by BatchDeliveryLatency(factor) session samples.  Records,
// meters and float64 rows stay those of the session-rate render.  Configuration, like BatchSetTrim: a checkpoint does not carry it, and
// the checkpoint, shard and master-finish calls refuse while a factor is in force; an error while a streamed job is open.
func (this *Context) BatchSetDelivery(factor int) error {
	return this.err(C.gdg_batch_set_delivery(this.ctx, C.int(factor)))
}

// BatchDelivery: the delivery factor in force (gdg_batch_delivery): 1 = off.
func (this *Context) BatchDelivery() int {
	return int(C.gdg_batch_delivery(this.ctx))
}

// BatchDeliveryLatency: the session samples a port delivered at factor lags the render by (gdg_batch_delivery_latency): 0, 38, 77.
func BatchDeliveryLatency(factor int) int {
	return int(C.gdg_batch_delivery_latency(C.int(factor)))
}

// DeliverTaps: the expanded anti-aliasing taps of a delivery factor (gdg_deliver_taps): 77 at 2, 155 at 4, none otherwise.
func DeliverTaps(factor int) []float64 {
	n := int(C.gdg_deliver_taps(C.int(factor), nil, 0))
	taps := make([]float64, n)
	if n > 0 {
		C.gdg_deliver_taps(C.int(factor), (*C.double)(unsafe.Pointer(&taps[0])), C.int(n))
	}
	return taps
}

// DeliverRows: nRows rows of samples float64 each, one after the other in rows, at 1 / factor of their rate (gdg_deliver_rows): samples
// is a positive multiple of factor.  history is nil (zeros in front of the first sample) or nRows * DeliverHistory values, read before and
// written after, so that consecutive calls continue a stream.
func (this *Context) DeliverRows(rows []float64, nRows int, samples int, factor int, history []float64) ([]float64, error) {
	if nRows <= 0 || samples <= 0 || factor <= 0 || len(rows) != nRows*samples {
		return nil, fmt.Errorf("gdg: %d values for %d rows of %d samples at factor %d", len(rows), nRows, samples, factor)
	}
	if history != nil && len(history) != nRows*DeliverHistory {
		return nil, fmt.Errorf("gdg: a history of %d values for %d rows", len(history), nRows)
	}
	out := make([]float64, nRows*(samples/factor))
	if len(out) == 0 {
		return nil, fmt.Errorf("gdg: %d samples at factor %d", samples, factor)
	}
	var hist *C.double
	if history != nil {
		hist = (*C.double)(unsafe.Pointer(&history[0]))
	}
	rc := C.gdg_deliver_rows(this.ctx, (*C.double)(unsafe.Pointer(&rows[0])), C.int(nRows), C.size_t(samples), C.int(factor), hist, (*C.double)(unsafe.Pointer(&out[0])))
	return out, this.err(rc)
}

// DeliverRowsDevice: the same on device memory, enqueued on the context's stream (gdg_deliver_rows_device): row r at dRows + r * rowStride,
// its delivered samples at dOut + r * outStride; dHistory nil or nRows * DeliverHistory doubles.
func (this *Context) DeliverRowsDevice(dRows unsafe.Pointer, rowStride int, nRows int, samples int, factor int, dHistory unsafe.Pointer, dOut unsafe.Pointer, outStride int) error {
	return this.err(C.gdg_deliver_rows_device(this.ctx, (*C.double)(dRows), C.size_t(rowStride), C.int(nRows), C.size_t(samples), C.int(factor), (*C.double)(dHistory), (*C.double)(dOut), C.size_t(outStride)))
}

// DeliverRatioHistory: the intermediate samples the ratio stage keeps from call to call (GDG_DELIVER_RATIO_HISTORY of the C header).
const DeliverRatioHistory = 127

// BatchSetDeliveryRatio: from the next batch call on every port leaves at (session rate / factor) * up / down (gdg_batch_set_out_ratio):
// the factor's decimator, then the polyphase ratio stage, in front of the encoders; 44.1 kHz from 192 is (4, 147, 160).  up / down is
// reduced, 1 <= up <= 160, 1 <= down <= 320, within a factor of two of 1; (factor, 1, 1) is BatchSetDelivery(factor).  An error while a
// streamed job is open; the checkpoint, shard and master-finish calls refuse while a ratio is in force.
func (this *Context) BatchSetDeliveryRatio(factor int, up int, down int) error {
	return this.err(C.gdg_batch_set_out_ratio(this.ctx, C.int(factor), C.int(up), C.int(down)))
}

// BatchDeliveryRatio: up and down of the delivery ratio in force (gdg_batch_out_ratio): 1, 1 = none.
func (this *Context) BatchDeliveryRatio() (int, int) {
	var up, down C.int
	C.gdg_batch_out_ratio(this.ctx, &up, &down)
	return int(up), int(down)
}

// BatchDeliverySamples: the delivered samples the session samples [first, first + count) produce (gdg_batch_out_samples): what an
// output buffer is sized with, per job and per streamed slice; 0 for anything inadmissible.
func BatchDeliverySamples(factor int, up int, down int, first int, count int) int {
	return int(C.gdg_batch_out_samples(C.int(factor), C.int(up), C.int(down), C.size_t(first), C.size_t(count)))
}

// BatchDeliveryRatioLatency: the session samples a port delivered at factor and up / down lags the render by (gdg_batch_out_ratio_latency).
func BatchDeliveryRatioLatency(factor int, up int, down int) int {
	return int(C.gdg_batch_out_ratio_latency(C.int(factor), C.int(up), C.int(down)))
}

// delivered: the delivered samples of the session samples [first, first + count) under the factor and the ratio in force.
func (this *Context) delivered(first int, count int) int {
	up, down := this.BatchDeliveryRatio()
	return BatchDeliverySamples(this.BatchDelivery(), up, down, first, count)
}

// DeliverRatioTaps: the ratio stage's table tap[up][T], row after row (gdg_out_ratio_taps); none for an inadmissible ratio and for 1/1.
func DeliverRatioTaps(up int, down int) []float64 {
	n := int(C.gdg_out_ratio_taps(C.int(up), C.int(down), nil, 0))
	taps := make([]float64, n)
	if n > 0 {
		C.gdg_out_ratio_taps(C.int(up), C.int(down), (*C.double)(unsafe.Pointer(&taps[0])), C.int(n))
	}
	return taps
}

// DeliverRowsRatio: nRows rows of samples intermediate samples each, the job's [first, first + samples), through the ratio stage
// (gdg_out_ratio_rows).  history is nil (zeros in front) or nRows * DeliverRatioHistory values, read before and written after, so that
// consecutive calls with advancing first continue a stream.
func (this *Context) DeliverRowsRatio(rows []float64, nRows int, samples int, up int, down int, first int, history []float64) ([]float64, error) {
	if nRows <= 0 || samples <= 0 || len(rows) != nRows*samples {
		return nil, fmt.Errorf("gdg: %d values for %d rows of %d samples at ratio %d/%d", len(rows), nRows, samples, up, down)
	}
	if history != nil && len(history) != nRows*DeliverRatioHistory {
		return nil, fmt.Errorf("gdg: a history of %d values for %d rows", len(history), nRows)
	}
	each := samples
	if up != 1 || down != 1 {
		each = BatchDeliverySamples(1, up, down, first, samples)
	}
	out := make([]float64, nRows*each+1)
	var hist *C.double
	if history != nil {
		hist = (*C.double)(unsafe.Pointer(&history[0]))
	}
	rc := C.gdg_out_ratio_rows(this.ctx, (*C.double)(unsafe.Pointer(&rows[0])), C.int(nRows), C.size_t(samples), C.int(up), C.int(down), C.size_t(first), hist, (*C.double)(unsafe.Pointer(&out[0])), C.size_t(each))
	return out[:nRows*each], this.err(rc)
}

// DeliverRowsRatioDevice: the same on device memory, enqueued on the context's stream (gdg_out_ratio_rows_device).
func (this *Context) DeliverRowsRatioDevice(dRows unsafe.Pointer, rowStride int, nRows int, samples int, up int, down int, first int, dHistory unsafe.Pointer, dOut unsafe.Pointer, outStride int) error {
	return this.err(C.gdg_out_ratio_rows_device(this.ctx, (*C.double)(dRows), C.size_t(rowStride), C.int(nRows), C.size_t(samples), C.int(up), C.int(down), C.size_t(first), (*C.double)(dHistory), (*C.double)(dOut), C.size_t(outStride)))
}

// WaveEncodeTrim: one mono row times gain through the encoder (gdg_wave_encode_trim): mode 0 the plain encoder, 1 the dithered one of
// WaveEncodeDither; sample i has index firstIndex + i.  gain 1 gives WaveEncodeDither's bytes.
func (this *Context) WaveEncodeTrim(format int, samples []float64, gain float64, mode int, seed uint64, port uint32, firstIndex uint64) ([]byte, error) {
	width := int(C.gdg_wave_bytes_per_sample(C.int(format)))
	if width == 0 {
		return nil, fmt.Errorf("gdg: unknown sample format %d", format)
	}
	data := make([]byte, len(samples)*width)
	if len(samples) == 0 {
		return data, nil
	}
	rc := C.gdg_wave_encode_trim(this.ctx, C.int(format), (*C.double)(unsafe.Pointer(&samples[0])), C.size_t(len(samples)), C.double(gain), C.int(mode), C.uint64_t(seed), C.uint32_t(port), C.uint64_t(firstIndex), unsafe.Pointer(&data[0]))
	return data, this.err(rc)
}

// WaveEncodeTrimDevice: the same on device memory, enqueued on the context's stream (gdg_wave_encode_trim_device): any 8-byte alignment
// of dSamples, any byte alignment of dBytes.
func (this *Context) WaveEncodeTrimDevice(format int, dSamples unsafe.Pointer, n int, gain float64, mode int, seed uint64, port uint32, firstIndex uint64, dBytes unsafe.Pointer) error {
	return this.err(C.gdg_wave_encode_trim_device(this.ctx, C.int(format), (*C.double)(dSamples), C.size_t(n), C.double(gain), C.int(mode), C.uint64_t(seed), C.uint32_t(port), C.uint64_t(firstIndex), unsafe.Pointer(dBytes)))
}

// TrimFromTruePeak: the gain of every port from its true-peak records (gdg_trim_from_true_peak), records[port][block] as BatchTruePeak
// hands them out: 1 for a silent port, else min(target / the port's largest TruePeak, maxGain).  Host arithmetic: no context and no
// device.  target and maxGain are finite and greater than 0; a NaN record is an error that names the port.
func TrimFromTruePeak(records [][]BlockTruePeak, target float64, maxGain float64) ([]float64, error) {
	ports := len(records)
	gain := make([]float64, ports)
	if ports == 0 {
		return gain, nil
	}
	blocks := len(records[0])
	for r, row := range records {
		if len(row) != blocks {
			return nil, fmt.Errorf("gdg: port %d has %d records, port 0 has %d", r, len(row), blocks)
		}
		for _, rec := range row {
			if rec.TruePeak != rec.TruePeak {
				return nil, fmt.Errorf("gdg: port %d has a NaN true peak", r)
			}
		}
	}
	rec := (*[1 << 26]C.gdg_block_true_peak)(C.calloc(C.size_t(ports*blocks+1), 16))
	if rec == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(rec))
	for r, row := range records {
		for b, v := range row {
			rec[r*blocks+b].true_peak = C.double(v.TruePeak)
			rec[r*blocks+b].position = C.uint32_t(v.Position)
			rec[r*blocks+b].overs = C.uint32_t(v.Overs)
		}
	}
	out := (*[1 << 28]C.double)(C.calloc(C.size_t(ports), 8))
	if out == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(out))
	if rc := C.gdg_trim_from_true_peak(&rec[0], C.int(ports), C.size_t(blocks), C.double(target), C.double(maxGain), &out[0]); rc != 0 {
		return nil, fmt.Errorf("gdg: gdg_trim_from_true_peak: %d (target and maxGain: finite and greater than 0)", int(rc))
	}
	for i := range gain {
		gain[i] = float64(out[i])
	}
	return gain, nil
}

// BlendTerm: one term of a blend output: a channel of the context (for BlendRows: a row) and its weight.
type BlendTerm struct {
	Channel int
	Weight  float64
}

// blendTable: the blends in gdg_batch_set_blends' CSR form, in C memory (first: len(blends)+1 offsets; channel, weight: one entry per term,
// one spare entry each so that a list without terms still has an address); release frees all three.
func blendTable(blends [][]BlendTerm) (first *[1 << 28]C.int, channel *[1 << 28]C.int, weight *[1 << 28]C.double, release func(), err error) {
	terms := 0
	for _, b := range blends {
		terms += len(b)
	}
	first = (*[1 << 28]C.int)(C.calloc(C.size_t(len(blends)+1), C.size_t(unsafe.Sizeof(C.int(0)))))
	channel = (*[1 << 28]C.int)(C.calloc(C.size_t(terms+1), C.size_t(unsafe.Sizeof(C.int(0)))))
	weight = (*[1 << 28]C.double)(C.calloc(C.size_t(terms+1), C.size_t(unsafe.Sizeof(C.double(0)))))
	release = func() {
		C.free(unsafe.Pointer(first))
		C.free(unsafe.Pointer(channel))
		C.free(unsafe.Pointer(weight))
	}
	if first == nil || channel == nil || weight == nil {
		release()
		return nil, nil, nil, func() {}, fmt.Errorf("gdg: out of memory")
	}
	k := 0
	for b, list := range blends {
		first[b] = C.int(k)
		for _, t := range list {
			channel[k] = C.int(t.Channel)
			weight[k] = C.double(t.Weight)
			k++
		}
	}
	first[len(blends)] = C.int(k)
	return first, channel, weight, release, nil
}

// BatchSetBlends: the blend outputs of the next batch calls (gdg_batch_set_blends).  Blend b is the sum of its terms over this context's
// chain output rows -- s = w0*x[c0], then s = s + wk*x[ck] in term order, every product and every add rounded on its own -- and port
// N + 3 + b of BatchRun and BatchStreamStep, behind the metronome's; all four record kinds hand out N + 3 + B ports.  gain has one output
// gain per blend (nil or empty: every gain 1).  1 to 32 terms per blend, at most 1024 blends, finite weights and gains; nil or an empty
// list turns the blends off.  Configuration, like BatchSetTrim: a checkpoint does not carry it -- set it again on the target of a resume --
// and an error while a streamed job is open.  The shard calls refuse a context with blends in force.
func (this *Context) BatchSetBlends(blends [][]BlendTerm, gain []float64) error {
	n := len(blends)
	if n == 0 {
		return this.err(C.gdg_batch_set_blends(this.ctx, 0, nil, nil, nil, nil))
	}
	if len(gain) != 0 && len(gain) != n {
		return fmt.Errorf("gdg: %d gains for %d blends", len(gain), n)
	}
	first, channel, weight, release, err := blendTable(blends)
	if err != nil {
		return err
	}
	defer release()
	if len(gain) == 0 {
		return this.err(C.gdg_batch_set_blends(this.ctx, C.int(n), &first[0], &channel[0], &weight[0], nil))
	}
	g := (*[1 << 28]C.double)(C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(C.double(0)))))
	if g == nil {
		return fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(g))
	for i, v := range gain {
		g[i] = C.double(v)
	}
	return this.err(C.gdg_batch_set_blends(this.ctx, C.int(n), &first[0], &channel[0], &weight[0], &g[0]))
}

// BatchBlends: the number of blends in force (gdg_batch_blends).
func (this *Context) BatchBlends() int {
	return int(C.gdg_batch_blends(this.ctx))
}

// BlendRows: the blends' sums over any rows of equal length (gdg_blend_rows); a term's Channel names a row.  result[blend][sample].
func (this *Context) BlendRows(rows [][]float64, blends [][]BlendTerm) ([][]float64, error) {
	n := len(rows)
	nb := len(blends)
	if n == 0 {
		return nil, fmt.Errorf("gdg: no rows")
	}
	samples := len(rows[0])
	var owned []unsafe.Pointer
	defer func() {
		for _, p := range owned {
			C.free(p)
		}
	}()
	rp := (*[1 << 20]*C.double)(C.calloc(C.size_t(n+nb+1), C.size_t(unsafe.Sizeof(uintptr(0)))))
	if rp == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	owned = append(owned, unsafe.Pointer(rp))
	for i := 0; i < n+nb; i++ {
		if i < n && len(rows[i]) != samples {
			return nil, fmt.Errorf("gdg: row %d has %d samples, row 0 has %d", i, len(rows[i]), samples)
		}
		p := C.calloc(C.size_t(samples+1), 8)
		if p == nil {
			return nil, fmt.Errorf("gdg: out of memory")
		}
		owned = append(owned, p)
		if i < n {
			copy((*[1 << 37]float64)(p)[:samples:samples], rows[i])
		}
		rp[i] = (*C.double)(p)
	}
	first, channel, weight, release, err := blendTable(blends)
	if err != nil {
		return nil, err
	}
	defer release()
	if e := this.err(C.gdg_blend_rows(this.ctx, &rp[0], C.int(n), C.size_t(samples), C.int(nb), &first[0], &channel[0], &weight[0], &rp[n])); e != nil {
		return nil, e
	}
	out := make([][]float64, nb)
	for b := range out {
		out[b] = make([]float64, samples)
		copy(out[b], (*[1 << 37]float64)(unsafe.Pointer(rp[n+b]))[:samples:samples])
	}
	return out, nil
}

// BlendRowsDevice: the same on device memory (gdg_blend_rows_device): row r at dRows + r*rowStride float64, blend b's sums at
// dOut + b*outStride (8-byte aligned, strides >= samples); returns when the sums are written.
func (this *Context) BlendRowsDevice(dRows unsafe.Pointer, rowStride int, nRows int, samples int, blends [][]BlendTerm, dOut unsafe.Pointer, outStride int) error {
	first, channel, weight, release, err := blendTable(blends)
	if err != nil {
		return err
	}
	defer release()
	return this.err(C.gdg_blend_rows_device(this.ctx, (*C.double)(dRows), C.size_t(rowStride), C.int(nRows), C.size_t(samples), C.int(len(blends)),
		&first[0], &channel[0], &weight[0], (*C.double)(dOut), C.size_t(outStride)))
}

// BlendMaxDelay: the largest delay of a blend's term in samples (GDG_BLEND_MAX_DELAY), and the samples of history a row keeps.
const BlendMaxDelay = 4096

// blendDelays: one delay per term of blends, in C memory with a spare entry (the caller frees it); delay[b][k] belongs to blends[b][k].
func blendDelays(blends [][]BlendTerm, delay [][]int) (unsafe.Pointer, error) {
	if len(delay) != len(blends) {
		return nil, fmt.Errorf("gdg: delays for %d blends, %d blends", len(delay), len(blends))
	}
	terms := 0
	for b, list := range blends {
		if len(delay[b]) != len(list) {
			return nil, fmt.Errorf("gdg: blend %d has %d terms and %d delays", b, len(list), len(delay[b]))
		}
		terms += len(list)
	}
	p := C.calloc(C.size_t(terms+1), 4)
	if p == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	dst := (*[1 << 28]C.int)(p)[:terms:terms]
	k := 0
	for _, list := range delay {
		for _, d := range list {
			dst[k] = C.int(d)
			k++
		}
	}
	return p, nil
}

// BatchSetBlendsDelayed: BatchSetBlends with one delay per term (gdg_batch_set_blends_delayed): term k of blend b reads its row
// delay[b][k] samples back, 0 to BlendMaxDelay, and zeros in front of the job; nil delays: every delay 0, which is BatchSetBlends.  While
// a delay is in force the context keeps the chain rows' last 4096 samples from step to step, the bytes do not depend on how the job is
// cut, and the checkpoint calls return an error: the history is not in the container.
func (this *Context) BatchSetBlendsDelayed(blends [][]BlendTerm, delay [][]int, gain []float64) error {
	n := len(blends)
	if n == 0 || delay == nil {
		return this.BatchSetBlends(blends, gain)
	}
	if len(gain) != 0 && len(gain) != n {
		return fmt.Errorf("gdg: %d gains for %d blends", len(gain), n)
	}
	dp, e := blendDelays(blends, delay)
	if e != nil {
		return e
	}
	defer C.free(dp)
	first, channel, weight, release, err := blendTable(blends)
	if err != nil {
		return err
	}
	defer release()
	if len(gain) == 0 {
		return this.err(C.gdg_batch_set_blends_delayed(this.ctx, C.int(n), &first[0], &channel[0], &weight[0], (*C.int)(dp), nil))
	}
	g := (*[1 << 28]C.double)(C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(C.double(0)))))
	if g == nil {
		return fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(g))
	for i, v := range gain {
		g[i] = C.double(v)
	}
	return this.err(C.gdg_batch_set_blends_delayed(this.ctx, C.int(n), &first[0], &channel[0], &weight[0], (*C.int)(dp), &g[0]))
}

// BatchBlendMaxDelay: the largest delay of the blends in force (gdg_batch_blend_max_delay); 0: the blends are stateless.
func (this *Context) BatchBlendMaxDelay() int {
	return int(C.gdg_batch_blend_max_delay(this.ctx))
}

// BlendRowsDelayed: the delayed blends' sums over any rows of equal length (gdg_blend_rows_delayed); history is nil (zeros in front of
// sample 0) or one run of BlendMaxDelay samples per row whose last entry is sample -1.  result[blend][sample].
func (this *Context) BlendRowsDelayed(rows [][]float64, blends [][]BlendTerm, delay [][]int, history [][]float64) ([][]float64, error) {
	n := len(rows)
	nb := len(blends)
	if n == 0 {
		return nil, fmt.Errorf("gdg: no rows")
	}
	if history != nil && len(history) != n {
		return nil, fmt.Errorf("gdg: %d histories for %d rows", len(history), n)
	}
	samples := len(rows[0])
	var owned []unsafe.Pointer
	defer func() {
		for _, p := range owned {
			C.free(p)
		}
	}()
	rp := (*[1 << 20]*C.double)(C.calloc(C.size_t(n+nb+1), C.size_t(unsafe.Sizeof(uintptr(0)))))
	if rp == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	owned = append(owned, unsafe.Pointer(rp))
	for i := 0; i < n+nb; i++ {
		if i < n && len(rows[i]) != samples {
			return nil, fmt.Errorf("gdg: row %d has %d samples, row 0 has %d", i, len(rows[i]), samples)
		}
		p := C.calloc(C.size_t(samples+1), 8)
		if p == nil {
			return nil, fmt.Errorf("gdg: out of memory")
		}
		owned = append(owned, p)
		if i < n {
			copy((*[1 << 37]float64)(p)[:samples:samples], rows[i])
		}
		rp[i] = (*C.double)(p)
	}
	hp := (*[1 << 20]*C.double)(C.calloc(C.size_t(n+1), C.size_t(unsafe.Sizeof(uintptr(0)))))
	if hp == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	owned = append(owned, unsafe.Pointer(hp))
	for i := range history {
		if len(history[i]) != BlendMaxDelay {
			return nil, fmt.Errorf("gdg: the history of row %d has %d samples; %d", i, len(history[i]), BlendMaxDelay)
		}
		p := C.calloc(C.size_t(BlendMaxDelay), 8)
		if p == nil {
			return nil, fmt.Errorf("gdg: out of memory")
		}
		owned = append(owned, p)
		copy((*[1 << 37]float64)(p)[:BlendMaxDelay:BlendMaxDelay], history[i])
		hp[i] = (*C.double)(p)
	}
	if delay == nil {
		delay = make([][]int, nb)
		for b := range delay {
			delay[b] = make([]int, len(blends[b]))
		}
	}
	dp, e := blendDelays(blends, delay)
	if e != nil {
		return nil, e
	}
	owned = append(owned, dp)
	first, channel, weight, release, err := blendTable(blends)
	if err != nil {
		return nil, err
	}
	defer release()
	var rc C.int
	if history == nil {
		rc = C.gdg_blend_rows_delayed(this.ctx, &rp[0], C.int(n), C.size_t(samples), C.int(nb), &first[0], &channel[0], &weight[0], (*C.int)(dp), nil, &rp[n])
	} else {
		rc = C.gdg_blend_rows_delayed(this.ctx, &rp[0], C.int(n), C.size_t(samples), C.int(nb), &first[0], &channel[0], &weight[0], (*C.int)(dp), &hp[0], &rp[n])
	}
	if e := this.err(rc); e != nil {
		return nil, e
	}
	out := make([][]float64, nb)
	for b := range out {
		out[b] = make([]float64, samples)
		copy(out[b], (*[1 << 37]float64)(unsafe.Pointer(rp[n+b]))[:samples:samples])
	}
	return out, nil
}

// BlendRowsDelayedDevice: the same on device memory (gdg_blend_rows_delayed_device): row r at dRows + r*rowStride float64, its history --
// nil, or BlendMaxDelay samples -- at dHistory + r*histStride, blend b's sums at dOut + b*outStride; returns when the sums are written.
func (this *Context) BlendRowsDelayedDevice(dRows unsafe.Pointer, rowStride int, nRows int, samples int, blends [][]BlendTerm, delay [][]int, dHistory unsafe.Pointer, histStride int, dOut unsafe.Pointer, outStride int) error {
	dp, e := blendDelays(blends, delay)
	if e != nil {
		return e
	}
	defer C.free(dp)
	first, channel, weight, release, err := blendTable(blends)
	if err != nil {
		return err
	}
	defer release()
	return this.err(C.gdg_blend_rows_delayed_device(this.ctx, (*C.double)(dRows), C.size_t(rowStride), C.int(nRows), C.size_t(samples), C.int(len(blends)),
		&first[0], &channel[0], &weight[0], (*C.int)(dp), (*C.double)(dHistory), C.size_t(histStride), (*C.double)(dOut), C.size_t(outStride)))
}

// BlendMaxTaps: the most taps of a blend's term (GDG_BLEND_MAX_TAPS).
const BlendMaxTaps = 64

// blendTaps: the taps of every term of blends in CSR form, in C memory with a spare entry each (the caller frees both); taps[b][k] belongs
// to blends[b][k], an empty list is a term without taps.
func blendTaps(blends [][]BlendTerm, taps [][][]float64) (unsafe.Pointer, unsafe.Pointer, error) {
	if len(taps) != len(blends) {
		return nil, nil, fmt.Errorf("gdg: taps for %d blends, %d blends", len(taps), len(blends))
	}
	terms := 0
	total := 0
	for b, list := range blends {
		if len(taps[b]) != len(list) {
			return nil, nil, fmt.Errorf("gdg: blend %d has %d terms and %d tap lists", b, len(list), len(taps[b]))
		}
		terms += len(list)
		for _, h := range taps[b] {
			total += len(h)
		}
	}
	fp := C.calloc(C.size_t(terms+2), 4)
	if fp == nil {
		return nil, nil, fmt.Errorf("gdg: out of memory")
	}
	tp := C.calloc(C.size_t(total+1), 8)
	if tp == nil {
		C.free(fp)
		return nil, nil, fmt.Errorf("gdg: out of memory")
	}
	first := (*[1 << 28]C.int)(fp)[: terms+1 : terms+1]
	dst := (*[1 << 28]C.double)(tp)[:total:total]
	k := 0
	at := 0
	for _, list := range taps {
		for _, h := range list {
			for _, v := range h {
				dst[at] = C.double(v)
				at++
			}
			k++
			first[k] = C.int(at)
		}
	}
	return fp, tp, nil
}

// BatchSetBlendsFiltered: BatchSetBlendsDelayed with a short FIR per term (gdg_batch_set_blends_filtered): term k of blend b reads its row
// through taps[b][k] -- up to BlendMaxTaps finite values, tap t on the sample delay[b][k] + t back -- and a term with an empty list is a
// delayed term.  A term reaches delay + max(taps, 1) - 1 samples back, BlendMaxDelay at the most.  nil taps: BatchSetBlendsDelayed.
func (this *Context) BatchSetBlendsFiltered(blends [][]BlendTerm, delay [][]int, taps [][][]float64, gain []float64) error {
	n := len(blends)
	if n == 0 || taps == nil {
		return this.BatchSetBlendsDelayed(blends, delay, gain)
	}
	if len(gain) != 0 && len(gain) != n {
		return fmt.Errorf("gdg: %d gains for %d blends", len(gain), n)
	}
	if delay == nil {
		delay = make([][]int, n)
		for b := range delay {
			delay[b] = make([]int, len(blends[b]))
		}
	}
	dp, e := blendDelays(blends, delay)
	if e != nil {
		return e
	}
	defer C.free(dp)
	fp, tp, e2 := blendTaps(blends, taps)
	if e2 != nil {
		return e2
	}
	defer C.free(fp)
	defer C.free(tp)
	first, channel, weight, release, err := blendTable(blends)
	if err != nil {
		return err
	}
	defer release()
	if len(gain) == 0 {
		return this.err(C.gdg_batch_set_blends_filtered(this.ctx, C.int(n), &first[0], &channel[0], &weight[0], (*C.int)(dp), (*C.int)(fp), (*C.double)(tp), nil))
	}
	g := (*[1 << 28]C.double)(C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(C.double(0)))))
	if g == nil {
		return fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(g))
	for i, v := range gain {
		g[i] = C.double(v)
	}
	return this.err(C.gdg_batch_set_blends_filtered(this.ctx, C.int(n), &first[0], &channel[0], &weight[0], (*C.int)(dp), (*C.int)(fp), (*C.double)(tp), &g[0]))
}

// BatchBlendMaxReach: how far back the blends in force read (gdg_batch_blend_max_reach): the largest delay + max(taps, 1) - 1; 0: stateless.
func (this *Context) BatchBlendMaxReach() int {
	return int(C.gdg_batch_blend_max_reach(this.ctx))
}

// BlendRowsFiltered: the filtered blends' sums over any rows of equal length (gdg_blend_rows_filtered); history as BlendRowsDelayed takes
// it.  result[blend][sample].
func (this *Context) BlendRowsFiltered(rows [][]float64, blends [][]BlendTerm, delay [][]int, taps [][][]float64, history [][]float64) ([][]float64, error) {
	n := len(rows)
	nb := len(blends)
	if n == 0 {
		return nil, fmt.Errorf("gdg: no rows")
	}
	if taps == nil {
		return this.BlendRowsDelayed(rows, blends, delay, history)
	}
	if history != nil && len(history) != n {
		return nil, fmt.Errorf("gdg: %d histories for %d rows", len(history), n)
	}
	samples := len(rows[0])
	var owned []unsafe.Pointer
	defer func() {
		for _, p := range owned {
			C.free(p)
		}
	}()
	rp := (*[1 << 20]*C.double)(C.calloc(C.size_t(n+nb+1), C.size_t(unsafe.Sizeof(uintptr(0)))))
	if rp == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	owned = append(owned, unsafe.Pointer(rp))
	for i := 0; i < n+nb; i++ {
		if i < n && len(rows[i]) != samples {
			return nil, fmt.Errorf("gdg: row %d has %d samples, row 0 has %d", i, len(rows[i]), samples)
		}
		p := C.calloc(C.size_t(samples+1), 8)
		if p == nil {
			return nil, fmt.Errorf("gdg: out of memory")
		}
		owned = append(owned, p)
		if i < n {
			copy((*[1 << 37]float64)(p)[:samples:samples], rows[i])
		}
		rp[i] = (*C.double)(p)
	}
	hp := (*[1 << 20]*C.double)(C.calloc(C.size_t(n+1), C.size_t(unsafe.Sizeof(uintptr(0)))))
	if hp == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	owned = append(owned, unsafe.Pointer(hp))
	for i := range history {
		if len(history[i]) != BlendMaxDelay {
			return nil, fmt.Errorf("gdg: the history of row %d has %d samples; %d", i, len(history[i]), BlendMaxDelay)
		}
		p := C.calloc(C.size_t(BlendMaxDelay), 8)
		if p == nil {
			return nil, fmt.Errorf("gdg: out of memory")
		}
		owned = append(owned, p)
		copy((*[1 << 37]float64)(p)[:BlendMaxDelay:BlendMaxDelay], history[i])
		hp[i] = (*C.double)(p)
	}
	if delay == nil {
		delay = make([][]int, nb)
		for b := range delay {
			delay[b] = make([]int, len(blends[b]))
		}
	}
	dp, e := blendDelays(blends, delay)
	if e != nil {
		return nil, e
	}
	owned = append(owned, dp)
	fp, tp, e2 := blendTaps(blends, taps)
	if e2 != nil {
		return nil, e2
	}
	owned = append(owned, fp, tp)
	first, channel, weight, release, err := blendTable(blends)
	if err != nil {
		return nil, err
	}
	defer release()
	var rc C.int
	if history == nil {
		rc = C.gdg_blend_rows_filtered(this.ctx, &rp[0], C.int(n), C.size_t(samples), C.int(nb), &first[0], &channel[0], &weight[0], (*C.int)(dp), (*C.int)(fp), (*C.double)(tp), nil, &rp[n])
	} else {
		rc = C.gdg_blend_rows_filtered(this.ctx, &rp[0], C.int(n), C.size_t(samples), C.int(nb), &first[0], &channel[0], &weight[0], (*C.int)(dp), (*C.int)(fp), (*C.double)(tp), &hp[0], &rp[n])
	}
	if e := this.err(rc); e != nil {
		return nil, e
	}
	out := make([][]float64, nb)
	for b := range out {
		out[b] = make([]float64, samples)
		copy(out[b], (*[1 << 37]float64)(unsafe.Pointer(rp[n+b]))[:samples:samples])
	}
	return out, nil
}

// BlendRowsFilteredDevice: the same on device memory (gdg_blend_rows_filtered_device), laid out as BlendRowsDelayedDevice takes it; returns
// when the sums are written.
func (this *Context) BlendRowsFilteredDevice(dRows unsafe.Pointer, rowStride int, nRows int, samples int, blends [][]BlendTerm, delay [][]int, taps [][][]float64, dHistory unsafe.Pointer, histStride int, dOut unsafe.Pointer, outStride int) error {
	dp, e := blendDelays(blends, delay)
	if e != nil {
		return e
	}
	defer C.free(dp)
	fp, tp, e2 := blendTaps(blends, taps)
	if e2 != nil {
		return e2
	}
	defer C.free(fp)
	defer C.free(tp)
	first, channel, weight, release, err := blendTable(blends)
	if err != nil {
		return err
	}
	defer release()
	return this.err(C.gdg_blend_rows_filtered_device(this.ctx, (*C.double)(dRows), C.size_t(rowStride), C.int(nRows), C.size_t(samples), C.int(len(blends)),
		&first[0], &channel[0], &weight[0], (*C.int)(dp), (*C.int)(fp), (*C.double)(tp), (*C.double)(dHistory), C.size_t(histStride), (*C.double)(dOut), C.size_t(outStride)))
}

// BlendFractionTaps: nTaps windowed-sinc taps (even, 2 to BlendMaxTaps) that delay by nTaps/2 - 1 + fraction samples, 0 <= fraction < 1,
// normalised to sum 1 (gdg_blend_fraction_taps); fraction 0 is the exact unit impulse.  Host arithmetic: no context and no device.
func BlendFractionTaps(nTaps int, fraction float64) ([]float64, error) {
	if nTaps < 2 || nTaps > BlendMaxTaps {
		return nil, fmt.Errorf("gdg: %d taps; an even count from 2 to %d", nTaps, BlendMaxTaps)
	}
	res := (*[1 << 28]C.double)(C.calloc(C.size_t(nTaps+1), 8))
	if res == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(res))
	if rc := C.gdg_blend_fraction_taps(C.int(nTaps), C.double(fraction), &res[0]); rc != 0 {
		return nil, fmt.Errorf("gdg: gdg_blend_fraction_taps: %d (%s)", int(rc), C.GoString(C.gdg_last_error(nil)))
	}
	taps := make([]float64, nTaps)
	for t := range taps {
		taps[t] = float64(res[t])
	}
	return taps, nil
}

// BlendDelaysFromAlign: delays and signs of the blends' terms from alignment records (gdg_blend_delays_from_align): records[port][block] as
// BatchAlign hands them out, measured with the reference list ref; a term's Channel names a port.  A port's lag is the lower median of Lag
// over its blocks with a normalised coefficient of at least minCoeff, its sign that of the sum of their Corr; delay[b][k] = the blend's
// largest lag - the term's, sign[b][k] = +1 or -1, to be multiplied into the weight.  Host arithmetic: no context and no device.  An
// error when the terms of a blend are not measured against one reference port.
func BlendDelaysFromAlign(records [][]BlockAlign, ref []int, minCoeff float64, blends [][]BlendTerm) ([][]int, [][]int, error) {
	ports := len(records)
	if ports == 0 || len(ref) != ports {
		return nil, nil, fmt.Errorf("gdg: %d references for %d ports", len(ref), ports)
	}
	blocks := len(records[0])
	for r, row := range records {
		if len(row) != blocks {
			return nil, nil, fmt.Errorf("gdg: port %d has %d records, port 0 has %d", r, len(row), blocks)
		}
	}
	rec := (*[1 << 25]C.gdg_block_align)(C.calloc(C.size_t(ports*blocks+1), 40))
	if rec == nil {
		return nil, nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(rec))
	for r, row := range records {
		for b, v := range row {
			rec[r*blocks+b].corr = C.double(v.Corr)
			rec[r*blocks+b].corr0 = C.double(v.Corr0)
			rec[r*blocks+b].ref_sq = C.double(v.RefSq)
			rec[r*blocks+b].sq_at_lag = C.double(v.SqAtLag)
			rec[r*blocks+b].lag = C.int32_t(v.Lag)
		}
	}
	fp, e := cRefs(ref)
	if e != nil {
		return nil, nil, e
	}
	defer C.free(fp)
	first, channel, weight, release, err := blendTable(blends)
	if err != nil {
		return nil, nil, err
	}
	defer release()
	terms := int(first[len(blends)])
	if weight == nil || terms < 0 {
		return nil, nil, fmt.Errorf("gdg: no blend table")
	}
	res := (*[1 << 28]C.int)(C.calloc(C.size_t(2*terms+2), 4))
	if res == nil {
		return nil, nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(res))
	if rc := C.gdg_blend_delays_from_align(&rec[0], C.int(ports), C.size_t(blocks), (*C.int)(fp), C.double(minCoeff), C.int(len(blends)), &first[0], &channel[0], &res[0], &res[terms+1]); rc != 0 {
		return nil, nil, fmt.Errorf("gdg: gdg_blend_delays_from_align: %d (the terms of a blend share one reference port; 0 <= minCoeff <= 1)", int(rc))
	}
	delay := make([][]int, len(blends))
	sign := make([][]int, len(blends))
	k := 0
	for b, list := range blends {
		delay[b] = make([]int, len(list))
		sign[b] = make([]int, len(list))
		for t := range list {
			delay[b][t] = int(res[k])
			sign[b][t] = int(res[terms+1+k])
			k++
		}
	}
	return delay, sign, nil
}

// BlockFit: one record of the blend fit (gdg_block_fit, 368 bytes in this layout): for one fit and one block the inner products a
// least-squares fit of blend weights needs.  Tt = sum t^2 of the target; Tx[k] = sum t*x_k; Xx holds the lower triangle of the terms' Gram
// matrix by rows, Xx[j*(j+1)/2+k] = sum x_j*x_k for k <= j.  Entries of terms >= Terms are 0.  Skipped counts the sample indices left out
// of every sum because one of the fit's rows was NaN or +-inf there.
type BlockFit struct {
	Tt      float64
	Tx      [8]float64
	Xx      [36]float64
	Skipped uint32
	Terms   uint32
}

// Fit: one fit of a list: the target port and 1 to 8 term ports.
type Fit struct {
	Target int
	Ports  []int
}

func goBlockFit(p unsafe.Pointer, fits int, blocks int) [][]BlockFit {
	out := make([][]BlockFit, fits)
	if fits*blocks == 0 {
		for f := range out {
			out[f] = []BlockFit{}
		}
		return out
	}
	recs := (*[1 << 22]BlockFit)(p)[: fits*blocks : fits*blocks]
	for f := range out {
		out[f] = make([]BlockFit, blocks)
		copy(out[f], recs[f*blocks:(f+1)*blocks])
	}
	return out
}

// fitTable: a list of fits in its CSR form in C memory -- first[len(fits)+1], then the ports, then the targets, one spare entry behind each --
// which the caller frees; the library validates it.
func fitTable(fits []Fit) (first *[1 << 28]C.int, port *[1 << 28]C.int, target *[1 << 28]C.int, release func()) {
	terms := 0
	for _, f := range fits {
		terms += len(f.Ports)
	}
	n := len(fits)
	p := C.calloc(C.size_t((n+2)+(terms+1)+(n+1)), 4)
	if p == nil {
		return nil, nil, nil, func() {}
	}
	all := (*[1 << 28]C.int)(p)
	first = (*[1 << 28]C.int)(unsafe.Pointer(&all[0]))
	port = (*[1 << 28]C.int)(unsafe.Pointer(&all[n+2]))
	target = (*[1 << 28]C.int)(unsafe.Pointer(&all[n+2+terms+1]))
	k := 0
	for i, f := range fits {
		first[i] = C.int(k)
		target[i] = C.int(f.Target)
		for _, v := range f.Ports {
			port[k] = C.int(v)
			k++
		}
	}
	first[n] = C.int(k)
	return first, port, target, func() { C.free(p) }
}

// BatchFitEnable: from the next batch call on, every batch call of the context keeps the fit records of what it rendered
// (gdg_batch_fit_enable): per fit a target port and 1 to 8 term ports of the call -- chain outputs, master left, master right, metronome,
// blend ports.  nil or an empty slice switches it off.  Configuration, like BatchSetBlends: a checkpoint does not carry it, and an error
// while a streamed job is open.
func (this *Context) BatchFitEnable(fits []Fit) error {
	if len(fits) == 0 {
		return this.err(C.gdg_batch_fit_enable(this.ctx, 0, nil, nil, nil))
	}
	first, port, target, release := fitTable(fits)
	if first == nil {
		return fmt.Errorf("gdg: out of memory")
	}
	defer release()
	return this.err(C.gdg_batch_fit_enable(this.ctx, C.int(len(fits)), &first[0], &port[0], &target[0]))
}

// BatchFits: the number of fits in force (gdg_batch_fits).
func (this *Context) BatchFits() int {
	return int(C.gdg_batch_fits(this.ctx))
}

// BatchFit: the fit records of the last completed batch call, result[fit][block] (gdg_batch_fit).  An error when the call ran without
// them, or was a master finish.
func (this *Context) BatchFit() ([][]BlockFit, error) {
	var fits C.int
	var blocks C.size_t
	if e := this.err(C.gdg_batch_fit(this.ctx, nil, 0, &fits, &blocks)); e != nil {
		return nil, e
	}
	n := int(fits) * int(blocks)
	if n == 0 {
		return goBlockFit(nil, int(fits), int(blocks)), nil
	}
	rec := C.calloc(C.size_t(n), 368)
	if rec == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(rec)
	if e := this.err(C.gdg_batch_fit(this.ctx, (*C.gdg_block_fit)(rec), C.size_t(n), &fits, &blocks)); e != nil {
		return nil, e
	}
	return goBlockFit(rec, int(fits), int(blocks)), nil
}

// BlockFitRows: the fit records of equally long host rows per block of `block` samples, the last one of a row possibly short
// (gdg_block_fit_rows); a fit's ports name rows; result[fit][block].
func (this *Context) BlockFitRows(rows [][]float64, block int, fits []Fit) ([][]BlockFit, error) {
	n := len(rows)
	if len(fits) == 0 {
		return [][]BlockFit{}, nil // as the C call: no fit, no record
	}
	if n == 0 || block < 1 {
		return nil, fmt.Errorf("gdg: %d rows, blocks of %d samples", n, block)
	}
	samples := len(rows[0])
	blocks := (samples + block - 1) / block
	var owned []unsafe.Pointer
	defer func() {
		for _, p := range owned {
			C.free(p)
		}
	}()
	first, port, target, release := fitTable(fits)
	if first == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	defer release()
	rp := (*[1 << 20]*C.double)(C.calloc(C.size_t(n), C.size_t(unsafe.Sizeof(uintptr(0)))))
	if rp == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	owned = append(owned, unsafe.Pointer(rp))
	for i, r := range rows {
		if len(r) != samples {
			return nil, fmt.Errorf("gdg: row %d has %d samples, row 0 has %d", i, len(r), samples)
		}
		p := C.malloc(C.size_t(samples*8 + 8))
		if p == nil {
			return nil, fmt.Errorf("gdg: out of memory")
		}
		owned = append(owned, p)
		copy((*[1 << 37]float64)(p)[:samples:samples], r)
		rp[i] = (*C.double)(p)
	}
	out := C.calloc(C.size_t(len(fits)*blocks+1), 368)
	if out == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	owned = append(owned, out)
	if e := this.err(C.gdg_block_fit_rows(this.ctx, &rp[0], C.int(n), C.size_t(samples), C.int(block), C.int(len(fits)), &first[0], &port[0], &target[0], (*C.gdg_block_fit)(out))); e != nil {
		return nil, e
	}
	return goBlockFit(out, len(fits), blocks), nil
}

// BlockFitRowsDevice: the same on device memory (gdg_block_fit_rows_device): row r at dRows + r*rowStride float64 (any 8-byte alignment,
// rowStride >= samples), the records into dRecords[len(fits)][ceil(samples/block)]; returns when they are written.
func (this *Context) BlockFitRowsDevice(dRows unsafe.Pointer, rowStride int, nRows int, samples int, block int, fits []Fit, dRecords unsafe.Pointer) error {
	if len(fits) == 0 {
		return nil // as the C call: no fit, no record
	}
	first, port, target, release := fitTable(fits)
	if first == nil {
		return fmt.Errorf("gdg: out of memory")
	}
	defer release()
	return this.err(C.gdg_block_fit_rows_device(this.ctx, (*C.double)(dRows), C.size_t(rowStride), C.int(nRows), C.size_t(samples), C.int(block), C.int(len(fits)), &first[0], &port[0], &target[0],
		(*C.gdg_block_fit)(dRecords)))
}

// BlendWeightsFromFit: the least-squares blend weights of every fit from its records (gdg_blend_weights_from_fit): records[fit][block] as
// BatchFit hands them out; (G + ridge*mean(diag G)*I) w = b by an unpivoted Cholesky factorisation in term order.  weights[fit] has the
// fit's Terms entries; residual[fit] is the share of the target's energy the fitted blend leaves.  Host arithmetic: no context and no
// device.  An error for a silent term, or a port used twice with ridge = 0.
func BlendWeightsFromFit(records [][]BlockFit, ridge float64) ([][]float64, []float64, error) {
	fits := len(records)
	if fits == 0 {
		return [][]float64{}, []float64{}, nil
	}
	blocks := len(records[0])
	for f, row := range records {
		if len(row) != blocks || blocks == 0 {
			return nil, nil, fmt.Errorf("gdg: fit %d has %d records, fit 0 has %d (at least 1)", f, len(row), blocks)
		}
	}
	rec := C.calloc(C.size_t(fits*blocks+1), 368)
	if rec == nil {
		return nil, nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(rec)
	dst := (*[1 << 22]BlockFit)(rec)[: fits*blocks : fits*blocks]
	for f, row := range records {
		copy(dst[f*blocks:(f+1)*blocks], row)
	}
	res := (*[1 << 28]C.double)(C.calloc(C.size_t(fits*9+1), 8))
	if res == nil {
		return nil, nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(res))
	if rc := C.gdg_blend_weights_from_fit((*C.gdg_block_fit)(rec), C.int(fits), C.size_t(blocks), C.double(ridge), &res[0], &res[fits*8]); rc != 0 {
		return nil, nil, fmt.Errorf("gdg: gdg_blend_weights_from_fit: %d (%s)", int(rc), C.GoString(C.gdg_last_error(nil)))
	}
	weights := make([][]float64, fits)
	residual := make([]float64, fits)
	for f := range weights {
		k := int(records[f][0].Terms)
		weights[f] = make([]float64, k)
		for t := 0; t < k; t++ {
			weights[f][t] = float64(res[f*8+t])
		}
		residual[f] = float64(res[fits*8+f])
	}
	return weights, residual, nil
}

// BlendFractionsFromFit: the fraction of a delay per fit from its records (gdg_blend_fractions_from_fit): records[fit][block] as BatchFit
// hands them out, every fit with the 2*steps - 1 candidates of one channel, term k at (k - (steps - 1)) / steps samples.  The candidate
// with the largest Tx[k] / sqrt(Xx[k][k]) over all blocks wins, the earlier on a tie; result[fit] is its k - (steps - 1), 0 for a silent
// target or no admissible candidate.  Host arithmetic: no context and no device.
func BlendFractionsFromFit(records [][]BlockFit, steps int) ([]int, error) {
	fits := len(records)
	if fits == 0 {
		return []int{}, nil
	}
	blocks := len(records[0])
	for f, row := range records {
		if len(row) != blocks || blocks == 0 {
			return nil, fmt.Errorf("gdg: fit %d has %d records, fit 0 has %d (at least 1)", f, len(row), blocks)
		}
	}
	rec := C.calloc(C.size_t(fits*blocks+1), 368)
	if rec == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(rec)
	dst := (*[1 << 22]BlockFit)(rec)[: fits*blocks : fits*blocks]
	for f, row := range records {
		copy(dst[f*blocks:(f+1)*blocks], row)
	}
	res := (*[1 << 28]C.int)(C.calloc(C.size_t(fits+1), 4))
	if res == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(res))
	if rc := C.gdg_blend_fractions_from_fit((*C.gdg_block_fit)(rec), C.int(fits), C.size_t(blocks), C.int(steps), &res[0]); rc != 0 {
		return nil, fmt.Errorf("gdg: gdg_blend_fractions_from_fit: %d (%s)", int(rc), C.GoString(C.gdg_last_error(nil)))
	}
	step := make([]int, fits)
	for f := range step {
		step[f] = int(res[f])
	}
	return step, nil
}

// GramIndex: the place of entry (i, j) in a Gram record -- the lower triangle by rows, the fit's Xx layout -- for either order of i and j.
func GramIndex(i int, j int) int {
	if j > i {
		return j*(j+1)/2 + i
	}
	return i*(i+1)/2 + j
}

// gramList: a list of ports in C memory, one spare entry behind it, which the caller frees; the library validates it.
func gramList(ports []int) (list *[1 << 28]C.int, release func()) {
	p := C.calloc(C.size_t(len(ports)+1), 4)
	if p == nil {
		return nil, func() {}
	}
	list = (*[1 << 28]C.int)(p)
	for i, v := range ports {
		list[i] = C.int(v)
	}
	return list, func() { C.free(p) }
}

func goGram(p unsafe.Pointer, blocks int, per int) [][]float64 {
	out := make([][]float64, blocks)
	if blocks*per == 0 {
		for b := range out {
			out[b] = []float64{}
		}
		return out
	}
	vals := (*[1 << 37]float64)(p)[: blocks*per : blocks*per]
	for b := range out {
		out[b] = make([]float64, per)
		copy(out[b], vals[b*per:(b+1)*per])
	}
	return out
}

// BatchGramEnable: from the next batch call on, every batch call of the context keeps the Gram records of what it rendered
// (gdg_batch_gram_enable): one list of 2 to 512 different ports of the call -- chain outputs, master left, master right, metronome, blend
// ports.  nil or an empty slice switches it off.  Configuration, like BatchFitEnable: a checkpoint does not carry it, and an error while a
// streamed job is open.
func (this *Context) BatchGramEnable(ports []int) error {
	if len(ports) == 0 {
		return this.err(C.gdg_batch_gram_enable(this.ctx, nil, 0))
	}
	list, release := gramList(ports)
	if list == nil {
		return fmt.Errorf("gdg: out of memory")
	}
	defer release()
	return this.err(C.gdg_batch_gram_enable(this.ctx, &list[0], C.int(len(ports))))
}

// BatchGramPorts: the Gram list in force (gdg_batch_gram_ports); empty: off.
func (this *Context) BatchGramPorts() []int {
	n := int(C.gdg_batch_gram_ports(this.ctx, nil, 0))
	out := make([]int, n)
	if n == 0 {
		return out
	}
	list, release := gramList(out)
	if list == nil {
		return []int{}
	}
	defer release()
	C.gdg_batch_gram_ports(this.ctx, &list[0], C.int(n))
	for i := range out {
		out[i] = int(list[i])
	}
	return out
}

// BatchGram: the Gram records of the last completed batch call, result[block][GramIndex(i, j)] with i and j positions in the list
// (gdg_batch_gram).  An error when the call ran without them, or was a master finish.
func (this *Context) BatchGram() ([][]float64, error) {
	var blocks C.size_t
	if e := this.err(C.gdg_batch_gram(this.ctx, nil, 0, &blocks)); e != nil {
		return nil, e
	}
	p := len(this.BatchGramPorts())
	per := p * (p + 1) / 2
	n := int(blocks) * per
	if n == 0 {
		return goGram(nil, int(blocks), per), nil
	}
	rec := (*[1 << 28]C.double)(C.calloc(C.size_t(n), 8))
	if rec == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(rec))
	if e := this.err(C.gdg_batch_gram(this.ctx, &rec[0], C.size_t(n), &blocks)); e != nil {
		return nil, e
	}
	return goGram(unsafe.Pointer(rec), int(blocks), per), nil
}

// BlockGramRows: the Gram records of equally long host rows per block of `block` samples, the last one of a row possibly short
// (gdg_block_gram_rows); ports names 1 to 512 different rows; result[block][GramIndex(i, j)].
func (this *Context) BlockGramRows(rows [][]float64, block int, ports []int) ([][]float64, error) {
	n := len(rows)
	if n == 0 || block < 1 || len(ports) == 0 {
		return nil, fmt.Errorf("gdg: %d rows, blocks of %d samples, %d ports", n, block, len(ports))
	}
	samples := len(rows[0])
	blocks := (samples + block - 1) / block
	per := len(ports) * (len(ports) + 1) / 2
	var owned []unsafe.Pointer
	defer func() {
		for _, p := range owned {
			C.free(p)
		}
	}()
	list, release := gramList(ports)
	if list == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	defer release()
	rp := (*[1 << 20]*C.double)(C.calloc(C.size_t(n), C.size_t(unsafe.Sizeof(uintptr(0)))))
	if rp == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	owned = append(owned, unsafe.Pointer(rp))
	for i, r := range rows {
		if len(r) != samples {
			return nil, fmt.Errorf("gdg: row %d has %d samples, row 0 has %d", i, len(r), samples)
		}
		p := C.malloc(C.size_t(samples*8 + 8))
		if p == nil {
			return nil, fmt.Errorf("gdg: out of memory")
		}
		owned = append(owned, p)
		copy((*[1 << 37]float64)(p)[:samples:samples], r)
		rp[i] = (*C.double)(p)
	}
	out := C.calloc(C.size_t(blocks*per+1), 8)
	if out == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	owned = append(owned, out)
	if e := this.err(C.gdg_block_gram_rows(this.ctx, &rp[0], C.int(n), C.size_t(samples), C.int(block), &list[0], C.int(len(ports)), (*C.double)(out))); e != nil {
		return nil, e
	}
	return goGram(out, blocks, per), nil
}

// BlockGramRowsDevice: the same on device memory (gdg_block_gram_rows_device): row r at dRows + r*rowStride float64 (any 8-byte alignment,
// rowStride >= samples), the records into dRecords[ceil(samples/block)][P*(P+1)/2]; returns when they are written.
func (this *Context) BlockGramRowsDevice(dRows unsafe.Pointer, rowStride int, nRows int, samples int, block int, ports []int, dRecords unsafe.Pointer) error {
	if len(ports) == 0 {
		return fmt.Errorf("gdg: no ports")
	}
	list, release := gramList(ports)
	if list == nil {
		return fmt.Errorf("gdg: out of memory")
	}
	defer release()
	return this.err(C.gdg_block_gram_rows_device(this.ctx, (*C.double)(dRows), C.size_t(rowStride), C.int(nRows), C.size_t(samples), C.int(block), &list[0], C.int(len(ports)),
		(*C.double)(dRecords)))
}

// BlendPickFromGram: up to maxTerms (1 to 8) of the candidates, picked greedily from Gram records so that their least-squares blend comes
// closest to the target (gdg_blend_pick_from_gram): records[block] as BatchGram hands them out for a list of nPorts ports; target and
// candidates are positions in that list.  picked holds list positions in pick order, weights their weights, residual[m] the share of the
// target's energy left after pick m.  Host arithmetic: no context and no device.  An error for a silent target, a NaN or inf entry, a
// repeated candidate.
func BlendPickFromGram(records [][]float64, nPorts int, target int, candidates []int, maxTerms int, ridge float64, minGain float64) ([]int, []float64, []float64, error) {
	blocks := len(records)
	per := nPorts * (nPorts + 1) / 2
	if blocks == 0 || nPorts < 2 || len(candidates) == 0 {
		return nil, nil, nil, fmt.Errorf("gdg: %d blocks (at least 1), %d ports (at least 2), %d candidates (at least 1)", blocks, nPorts, len(candidates))
	}
	for b, row := range records {
		if len(row) != per {
			return nil, nil, nil, fmt.Errorf("gdg: record %d has %d entries, %d ports make %d", b, len(row), nPorts, per)
		}
	}
	rec := (*[1 << 28]C.double)(C.calloc(C.size_t(blocks*per+1), 8))
	if rec == nil {
		return nil, nil, nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(rec))
	for b, row := range records {
		for e, v := range row {
			rec[b*per+e] = C.double(v)
		}
	}
	list, release := gramList(candidates)
	if list == nil {
		return nil, nil, nil, fmt.Errorf("gdg: out of memory")
	}
	defer release()
	res := (*[1 << 28]C.double)(C.calloc(17, 8))
	if res == nil {
		return nil, nil, nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(res))
	got, releaseGot := gramList(make([]int, 8))
	if got == nil {
		return nil, nil, nil, fmt.Errorf("gdg: out of memory")
	}
	defer releaseGot()
	var n C.int
	if rc := C.gdg_blend_pick_from_gram(&rec[0], C.int(nPorts), C.size_t(blocks), C.int(target), &list[0], C.int(len(candidates)), C.int(maxTerms), C.double(ridge), C.double(minGain),
		&got[0], &res[0], &res[8], &n); rc != 0 {
		return nil, nil, nil, fmt.Errorf("gdg: gdg_blend_pick_from_gram: %d (%s)", int(rc), C.GoString(C.gdg_last_error(nil)))
	}
	picked := make([]int, int(n))
	weights := make([]float64, int(n))
	residual := make([]float64, int(n))
	for m := range picked {
		picked[m] = int(got[m])
		weights[m] = float64(res[m])
		residual[m] = float64(res[8+m])
	}
	return picked, weights, residual, nil
}

// TapFit: one tap fit of a list: the target port, 1 to 4 term ports and the taps per term (1 to 64, ports x taps at most 128).
type TapFit struct {
	Target int
	Ports  []int
	Taps   int
}

// tapFitTable: a list of tap fits in its CSR form in C memory -- first[len(fits)+1], the ports, the targets, the taps, one spare entry behind
// each -- which the caller frees; the library validates it.
func tapFitTable(fits []TapFit) (first *[1 << 28]C.int, port *[1 << 28]C.int, target *[1 << 28]C.int, taps *[1 << 28]C.int, release func()) {
	terms := 0
	for _, f := range fits {
		terms += len(f.Ports)
	}
	n := len(fits)
	p := C.calloc(C.size_t((n+2)+(terms+1)+(n+1)+(n+1)), 4)
	if p == nil {
		return nil, nil, nil, nil, func() {}
	}
	all := (*[1 << 28]C.int)(p)
	first = (*[1 << 28]C.int)(unsafe.Pointer(&all[0]))
	port = (*[1 << 28]C.int)(unsafe.Pointer(&all[n+2]))
	target = (*[1 << 28]C.int)(unsafe.Pointer(&all[n+2+terms+1]))
	taps = (*[1 << 28]C.int)(unsafe.Pointer(&all[n+2+terms+1+n+1]))
	k := 0
	for i, f := range fits {
		first[i] = C.int(k)
		target[i] = C.int(f.Target)
		taps[i] = C.int(f.Taps)
		for _, v := range f.Ports {
			port[k] = C.int(v)
			k++
		}
	}
	first[n] = C.int(k)
	return first, port, target, taps, func() { C.free(p) }
}

// TapFitDoubles: D, the doubles of one block's tap-fit record (gdg_tapfit_doubles): the sum over the fits of V*(V+1)/2, V = ports x taps + 1.
func TapFitDoubles(fits []TapFit) int {
	if len(fits) == 0 {
		return 0
	}
	first, _, _, taps, release := tapFitTable(fits)
	if first == nil {
		return 0
	}
	defer release()
	return int(C.gdg_tapfit_doubles(C.int(len(fits)), &first[0], &taps[0]))
}

// BatchTapFitEnable: from the next batch call on, every batch call of the context keeps the tap-fit records of what it rendered
// (gdg_batch_tapfit_enable).  nil or an empty slice switches it off.  Configuration, like BatchFitEnable: a checkpoint does not carry it,
// and an error while a streamed job is open.
func (this *Context) BatchTapFitEnable(fits []TapFit) error {
	if len(fits) == 0 {
		return this.err(C.gdg_batch_tapfit_enable(this.ctx, 0, nil, nil, nil, nil))
	}
	first, port, target, taps, release := tapFitTable(fits)
	if first == nil {
		return fmt.Errorf("gdg: out of memory")
	}
	defer release()
	return this.err(C.gdg_batch_tapfit_enable(this.ctx, C.int(len(fits)), &first[0], &port[0], &target[0], &taps[0]))
}

// BatchTapFits: the number of tap fits in force (gdg_batch_tapfits).
func (this *Context) BatchTapFits() int {
	return int(C.gdg_batch_tapfits(this.ctx))
}

// BatchTapFit: the tap-fit records of the last completed batch call, result[block][D] (gdg_batch_tapfit).  An error when the call ran
// without them, or was a master finish.
func (this *Context) BatchTapFit() ([][]float64, error) {
	var blocks C.size_t
	var per C.size_t
	if e := this.err(C.gdg_batch_tapfit(this.ctx, nil, 0, &blocks, &per)); e != nil {
		return nil, e
	}
	n := int(blocks) * int(per)
	if n == 0 {
		return goGram(nil, int(blocks), int(per)), nil
	}
	rec := (*[1 << 28]C.double)(C.calloc(C.size_t(n), 8))
	if rec == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(rec))
	if e := this.err(C.gdg_batch_tapfit(this.ctx, &rec[0], C.size_t(n), &blocks, &per)); e != nil {
		return nil, e
	}
	return goGram(unsafe.Pointer(rec), int(blocks), int(per)), nil
}

// BlockTapFitRows: the tap-fit records of equally long host rows per block of `block` samples, the last one of a row possibly short
// (gdg_block_tapfit_rows); a fit's ports name rows; result[block][D].
func (this *Context) BlockTapFitRows(rows [][]float64, block int, fits []TapFit) ([][]float64, error) {
	n := len(rows)
	if len(fits) == 0 {
		return [][]float64{}, nil // as the C call: no fit, no record
	}
	if n == 0 || block < 1 {
		return nil, fmt.Errorf("gdg: %d rows, blocks of %d samples", n, block)
	}
	samples := len(rows[0])
	blocks := (samples + block - 1) / block
	per := TapFitDoubles(fits)
	var owned []unsafe.Pointer
	defer func() {
		for _, p := range owned {
			C.free(p)
		}
	}()
	first, port, target, taps, release := tapFitTable(fits)
	if first == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	defer release()
	rp := (*[1 << 20]*C.double)(C.calloc(C.size_t(n), C.size_t(unsafe.Sizeof(uintptr(0)))))
	if rp == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	owned = append(owned, unsafe.Pointer(rp))
	for i, r := range rows {
		if len(r) != samples {
			return nil, fmt.Errorf("gdg: row %d has %d samples, row 0 has %d", i, len(r), samples)
		}
		p := C.malloc(C.size_t(samples*8 + 8))
		if p == nil {
			return nil, fmt.Errorf("gdg: out of memory")
		}
		owned = append(owned, p)
		copy((*[1 << 37]float64)(p)[:samples:samples], r)
		rp[i] = (*C.double)(p)
	}
	out := C.calloc(C.size_t(blocks*per+1), 8)
	if out == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	owned = append(owned, out)
	if e := this.err(C.gdg_block_tapfit_rows(this.ctx, &rp[0], C.int(n), C.size_t(samples), C.int(block), C.int(len(fits)), &first[0], &port[0], &target[0], &taps[0], (*C.double)(out))); e != nil {
		return nil, e
	}
	return goGram(out, blocks, per), nil
}

// BlockTapFitRowsDevice: the same on device memory (gdg_block_tapfit_rows_device): row r at dRows + r*rowStride float64 (any 8-byte
// alignment, rowStride >= samples), the records into dRecords[ceil(samples/block)][D]; returns when they are written.
func (this *Context) BlockTapFitRowsDevice(dRows unsafe.Pointer, rowStride int, nRows int, samples int, block int, fits []TapFit, dRecords unsafe.Pointer) error {
	if len(fits) == 0 {
		return nil // as the C call: no fit, no record
	}
	first, port, target, taps, release := tapFitTable(fits)
	if first == nil {
		return fmt.Errorf("gdg: out of memory")
	}
	defer release()
	return this.err(C.gdg_block_tapfit_rows_device(this.ctx, (*C.double)(dRows), C.size_t(rowStride), C.int(nRows), C.size_t(samples), C.int(block), C.int(len(fits)), &first[0], &port[0], &target[0], &taps[0],
		(*C.double)(dRecords)))
}

// BlendTapsFromTapFit: the least-squares taps of every fit from its records (gdg_blend_taps_from_tapfit): records[block] as BatchTapFit hands
// them out; (A + ridge*mean(diag A)*I) h = b by an unpivoted Cholesky factorisation in virtual-row order.  taps[fit][term] has the fit's Taps
// entries, lag ascending -- the taps of a filtered blend term; residual[fit] is the share of the target's energy the fitted filters leave.
// Host arithmetic: no context and no device.  An error, with fit, term and lag named, for a pivot at or below the bound -- a silent or
// band-limited term, a port used twice: try ridge > 0 -- and for a NaN or inf entry.
func BlendTapsFromTapFit(records [][]float64, fits []TapFit, ridge float64) ([][][]float64, []float64, error) {
	blocks := len(records)
	per := TapFitDoubles(fits)
	if blocks == 0 || len(fits) == 0 {
		return nil, nil, fmt.Errorf("gdg: %d blocks (at least 1), %d fits (at least 1)", blocks, len(fits))
	}
	total := 0
	for _, f := range fits {
		total += len(f.Ports) * f.Taps
	}
	for b, row := range records {
		if len(row) != per {
			return nil, nil, fmt.Errorf("gdg: record %d has %d entries, the fits make %d", b, len(row), per)
		}
	}
	rec := (*[1 << 28]C.double)(C.calloc(C.size_t(blocks*per+1), 8))
	if rec == nil {
		return nil, nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(rec))
	for b, row := range records {
		for e, v := range row {
			rec[b*per+e] = C.double(v)
		}
	}
	first, _, _, taps, release := tapFitTable(fits)
	if first == nil {
		return nil, nil, fmt.Errorf("gdg: out of memory")
	}
	defer release()
	res := (*[1 << 28]C.double)(C.calloc(C.size_t(total+len(fits)+1), 8))
	if res == nil {
		return nil, nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(res))
	if rc := C.gdg_blend_taps_from_tapfit(&rec[0], C.int(len(fits)), &first[0], &taps[0], C.size_t(blocks), C.double(ridge), &res[0], &res[total]); rc != 0 {
		return nil, nil, fmt.Errorf("gdg: gdg_blend_taps_from_tapfit: %d (%s)", int(rc), C.GoString(C.gdg_last_error(nil)))
	}
	out := make([][][]float64, len(fits))
	residual := make([]float64, len(fits))
	at := 0
	for f, fit := range fits {
		out[f] = make([][]float64, len(fit.Ports))
		for j := range fit.Ports {
			out[f][j] = make([]float64, fit.Taps)
			for a := range out[f][j] {
				out[f][j][a] = float64(res[at])
				at++
			}
		}
		residual[f] = float64(res[total+f])
	}
	return out, residual, nil
}

// TransferPair: one (port, target) pair of a transfer list: the port whose spectrum is measured and the target it is measured against.
type TransferPair struct {
	Port   int
	Target int
}

// transferLists: the pairs as the two C int lists of the transfer calls (one spare entry behind each), and what frees them.
func transferLists(pairs []TransferPair) (port *[1 << 28]C.int, target *[1 << 28]C.int, release func()) {
	port = (*[1 << 28]C.int)(C.calloc(C.size_t(len(pairs)+1), 4))
	target = (*[1 << 28]C.int)(C.calloc(C.size_t(len(pairs)+1), 4))
	release = func() {
		C.free(unsafe.Pointer(port))
		C.free(unsafe.Pointer(target))
	}
	if port == nil || target == nil {
		release()
		return nil, nil, func() {}
	}
	for i, p := range pairs {
		port[i] = C.int(p.Port)
		target[i] = C.int(p.Target)
	}
	return port, target, release
}

// TransferDoubles: the doubles of one block's transfer record (gdg_transfer_doubles): nPairs * (4096/group + 1) * 4; 0 for no pair or a
// group width that is none of 1, 2, 4 .. 64.
func TransferDoubles(nPairs int, group int) int {
	return int(C.gdg_transfer_doubles(C.int(nPairs), C.int(group)))
}

// BatchTransferEnable: from the next batch call on, every batch call of the context keeps the transfer records of what it rendered
// (gdg_batch_transfer_enable): per block and pair the auto-spectra and the cross-spectrum in groups of `group` bins.  nil or an empty
// slice switches it off.  Configuration, like BatchTapFitEnable: a checkpoint does not carry it, and it is refused while a streamed job is open.
func (this *Context) BatchTransferEnable(pairs []TransferPair, group int) error {
	if len(pairs) == 0 {
		return this.err(C.gdg_batch_transfer_enable(this.ctx, 0, nil, nil, C.int(group)))
	}
	port, target, release := transferLists(pairs)
	if port == nil {
		return fmt.Errorf("gdg: out of memory")
	}
	defer release()
	return this.err(C.gdg_batch_transfer_enable(this.ctx, C.int(len(pairs)), &port[0], &target[0], C.int(group)))
}

// BatchTransfers: the number of transfer pairs in force (gdg_batch_transfers).
func (this *Context) BatchTransfers() int {
	return int(C.gdg_batch_transfers(this.ctx))
}

// BatchTransfer: the transfer records of the last completed batch call, result[block][nPairs*G*4] (gdg_batch_transfer).  An error when the
// call ran without them, or was a master finish.
func (this *Context) BatchTransfer() ([][]float64, error) {
	var blocks C.size_t
	var per C.size_t
	if e := this.err(C.gdg_batch_transfer(this.ctx, nil, 0, &blocks, &per)); e != nil {
		return nil, e
	}
	n := int(blocks) * int(per)
	if n == 0 {
		return goGram(nil, int(blocks), int(per)), nil
	}
	rec := (*[1 << 28]C.double)(C.calloc(C.size_t(n), 8))
	if rec == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(rec))
	if e := this.err(C.gdg_batch_transfer(this.ctx, &rec[0], C.size_t(n), &blocks, &per)); e != nil {
		return nil, e
	}
	return goGram(unsafe.Pointer(rec), int(blocks), int(per)), nil
}

// BlockTransferRows: the transfer records of equally long host rows per block of 8192 samples, the last one of a row possibly short
// (gdg_block_transfer_rows); a pair's ports name rows; result[block][nPairs*G*4].
func (this *Context) BlockTransferRows(rows [][]float64, pairs []TransferPair, group int) ([][]float64, error) {
	n := len(rows)
	if n == 0 || len(pairs) == 0 {
		return nil, fmt.Errorf("gdg: %d rows, %d pairs", n, len(pairs))
	}
	samples := len(rows[0])
	blocks := (samples + 8191) / 8192
	per := TransferDoubles(len(pairs), group)
	var owned []unsafe.Pointer
	defer func() {
		for _, p := range owned {
			C.free(p)
		}
	}()
	port, target, release := transferLists(pairs)
	if port == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	defer release()
	rp := (*[1 << 20]*C.double)(C.calloc(C.size_t(n), C.size_t(unsafe.Sizeof(uintptr(0)))))
	if rp == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	owned = append(owned, unsafe.Pointer(rp))
	for i, r := range rows {
		if len(r) != samples {
			return nil, fmt.Errorf("gdg: row %d has %d samples, row 0 has %d", i, len(r), samples)
		}
		p := C.malloc(C.size_t(samples*8 + 8))
		if p == nil {
			return nil, fmt.Errorf("gdg: out of memory")
		}
		owned = append(owned, p)
		copy((*[1 << 37]float64)(p)[:samples:samples], r)
		rp[i] = (*C.double)(p)
	}
	out := C.calloc(C.size_t(blocks*per+1), 8)
	if out == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	owned = append(owned, out)
	if e := this.err(C.gdg_block_transfer_rows(this.ctx, &rp[0], C.int(n), C.size_t(samples), C.int(len(pairs)), &port[0], &target[0], C.int(group), (*C.double)(out))); e != nil {
		return nil, e
	}
	return goGram(out, blocks, per), nil
}

// BlockTransferRowsDevice: the same on device memory (gdg_block_transfer_rows_device): row r at dRows + r*rowStride float64 (any 8-byte
// alignment, rowStride >= samples), the records into dRecords[ceil(samples/8192)][nPairs*G*4]; returns when they are written.
func (this *Context) BlockTransferRowsDevice(dRows unsafe.Pointer, rowStride int, nRows int, samples int, pairs []TransferPair, group int, dRecords unsafe.Pointer) error {
	port, target, release := transferLists(pairs)
	if port == nil {
		return fmt.Errorf("gdg: out of memory")
	}
	defer release()
	return this.err(C.gdg_block_transfer_rows_device(this.ctx, (*C.double)(dRows), C.size_t(rowStride), C.int(nRows), C.size_t(samples), C.int(len(pairs)), &port[0], &target[0], C.int(group),
		(*C.double)(dRecords)))
}

// MatchTapsFromTransfer: the match taps of every pair from its records (gdg_match_taps_from_transfer): records[block] as BatchTransfer hands
// them out; H = Sxy / (Sxx + ridge*mean Sxx) over the summed blocks, its inverse real transform of length 8192/group, nTaps of it around
// `center` under a raised-cosine taper.  taps[pair] has nTaps entries -- an impulse response like any other; coherence[pair] is the share of
// the target's energy a linear filter on the port explains.  Host arithmetic: no context and no device.  An error, with the pair named,
// for a NaN or inf entry and for a pair with no energy in its port.
func MatchTapsFromTransfer(records [][]float64, nPairs int, group int, ridge float64, nTaps int, center int) ([][]float64, []float64, error) {
	blocks := len(records)
	per := TransferDoubles(nPairs, group)
	if blocks == 0 || per == 0 || nTaps < 1 {
		return nil, nil, fmt.Errorf("gdg: %d blocks (at least 1), %d pairs in groups of %d, %d taps", blocks, nPairs, group, nTaps)
	}
	for b, row := range records {
		if len(row) != per {
			return nil, nil, fmt.Errorf("gdg: record %d has %d entries, the pairs make %d", b, len(row), per)
		}
	}
	rec := (*[1 << 28]C.double)(C.calloc(C.size_t(blocks*per+1), 8))
	if rec == nil {
		return nil, nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(rec))
	for b, row := range records {
		for e, v := range row {
			rec[b*per+e] = C.double(v)
		}
	}
	total := nPairs * nTaps
	res := (*[1 << 28]C.double)(C.calloc(C.size_t(total+nPairs+1), 8))
	if res == nil {
		return nil, nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(res))
	if rc := C.gdg_match_taps_from_transfer(&rec[0], C.int(nPairs), C.int(group), C.size_t(blocks), C.double(ridge), C.int(nTaps), C.int(center), &res[0], &res[total]); rc != 0 {
		return nil, nil, fmt.Errorf("gdg: gdg_match_taps_from_transfer: %d (%s)", int(rc), C.GoString(C.gdg_last_error(nil)))
	}
	taps := make([][]float64, nPairs)
	coherence := make([]float64, nPairs)
	for p := range taps {
		taps[p] = make([]float64, nTaps)
		for m := range taps[p] {
			taps[p][m] = float64(res[p*nTaps+m])
		}
		coherence[p] = float64(res[total+p])
	}
	return taps, coherence, nil
}

// BlockDelivered: one record of a delivered block (gdg_block_delivered; include/gdg.h, DELIVERED RECORDS): the samples' peak, sum of squares
// and clipped count in the block statistics' order at the block's length, and a true peak over the block's samples and the interpolated
// points that complete in it -- seamless across blocks.  Position = 4*(n - o) + phase of the first point that attains TruePeak, o the
// block's first sample; it can be as low as -47.
type BlockDelivered struct {
	TruePeak  float64
	Peak      float64
	SumSq     float64
	Position  int32
	PeakIndex uint32
	Overs     uint32
	Clipped   uint32
}

func goBlockDelivered(p unsafe.Pointer, rows int, blocks int) [][]BlockDelivered {
	out := make([][]BlockDelivered, rows)
	if rows*blocks == 0 {
		for r := range out {
			out[r] = []BlockDelivered{}
		}
		return out
	}
	recs := (*[1 << 25]C.gdg_block_delivered)(p)[: rows*blocks : rows*blocks]
	for r := range out {
		out[r] = make([]BlockDelivered, blocks)
		for b := range out[r] {
			c := recs[r*blocks+b]
			out[r][b] = BlockDelivered{float64(c.true_peak), float64(c.peak), float64(c.sum_sq), int32(c.position), uint32(c.peak_index), uint32(c.overs), uint32(c.clipped)}
		}
	}
	return out
}

// BlockDeliveredRows: the records of equally long host rows cut into blocks by span[0 .. nBlocks] -- ascending, span[0] = 0, the last the
// rows' length, every block 1 to 16384 samples (gdg_block_out_rows); result[row][block].  history: nil (zeros stand in front of the rows,
// nothing is kept) or nRows*23 float64, the newest last, read before and written after: two calls that continue each other through it give
// the records of the one call.
func (this *Context) BlockDeliveredRows(rows [][]float64, span []int, history []float64) ([][]BlockDelivered, error) {
	n := len(rows)
	if n == 0 || len(span) < 2 {
		return nil, fmt.Errorf("gdg: BlockDeliveredRows needs rows and the spans of at least one block")
	}
	if history != nil && len(history) != n*23 {
		return nil, fmt.Errorf("gdg: a history of %d values for %d rows; 23 per row", len(history), n)
	}
	samples := len(rows[0])
	blocks := len(span) - 1
	var owned []unsafe.Pointer
	defer func() {
		for _, p := range owned {
			C.free(p)
		}
	}()
	rp := (*[1 << 20]*C.double)(C.calloc(C.size_t(n), C.size_t(unsafe.Sizeof(uintptr(0)))))
	if rp == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	owned = append(owned, unsafe.Pointer(rp))
	for i, r := range rows {
		if len(r) != samples {
			return nil, fmt.Errorf("gdg: row %d has %d samples, row 0 has %d", i, len(r), samples)
		}
		p := C.malloc(C.size_t(samples*8 + 8))
		if p == nil {
			return nil, fmt.Errorf("gdg: out of memory")
		}
		owned = append(owned, p)
		copy((*[1 << 37]float64)(p)[:samples:samples], r)
		rp[i] = (*C.double)(p)
	}
	sp := (*[1 << 28]C.size_t)(C.calloc(C.size_t(len(span)), 8))
	if sp == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	owned = append(owned, unsafe.Pointer(sp))
	for i, v := range span {
		if v < 0 {
			return nil, fmt.Errorf("gdg: span %d is %d", i, v)
		}
		sp[i] = C.size_t(v)
	}
	var hp *C.double
	if history != nil {
		h := C.malloc(C.size_t(n * 23 * 8))
		if h == nil {
			return nil, fmt.Errorf("gdg: out of memory")
		}
		owned = append(owned, h)
		copy((*[1 << 30]float64)(h)[:n*23:n*23], history)
		hp = (*C.double)(h)
	}
	out := C.calloc(C.size_t(n*blocks+1), 40)
	if out == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	owned = append(owned, out)
	if e := this.err(C.gdg_block_out_rows(this.ctx, &rp[0], C.int(n), C.size_t(samples), &sp[0], C.size_t(blocks), hp, (*C.gdg_block_delivered)(out))); e != nil {
		return nil, e
	}
	if history != nil {
		copy(history, (*[1 << 30]float64)(unsafe.Pointer(hp))[:n*23:n*23])
	}
	return goBlockDelivered(out, n, blocks), nil
}

// BlockDeliveredRowsDevice: the same on device memory, enqueued on the context's stream (gdg_block_out_rows_device): row r at
// dRows + r*rowStride float64 (any 8-byte alignment, rowStride >= samples), span a host slice, dHistory nil or nRows*23 float64 on the
// device, the records into dRecords[nRows][len(span)-1].
func (this *Context) BlockDeliveredRowsDevice(dRows unsafe.Pointer, rowStride int, nRows int, samples int, span []int, dHistory unsafe.Pointer, dRecords unsafe.Pointer) error {
	if len(span) < 2 {
		return fmt.Errorf("gdg: BlockDeliveredRowsDevice needs the spans of at least one block")
	}
	sp := (*[1 << 28]C.size_t)(C.calloc(C.size_t(len(span)), 8))
	if sp == nil {
		return fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(sp))
	for i, v := range span {
		if v < 0 {
			return fmt.Errorf("gdg: span %d is %d", i, v)
		}
		sp[i] = C.size_t(v)
	}
	return this.err(C.gdg_block_out_rows_device(this.ctx, (*C.double)(dRows), C.size_t(rowStride), C.int(nRows), C.size_t(samples), &sp[0], C.size_t(len(span)-1),
		(*C.double)(dHistory), (*C.gdg_block_delivered)(dRecords)))
}

// BatchDeliveredEnable: from the next batch call on, BatchRun and BatchStreamStep keep the records of the rows the encoders read -- the
// delivered rows, in front of the trim and blend gains -- of every encoded port (gdg_batch_out_records_enable); off by default.
// Configuration: a checkpoint does not carry it, an error while a streamed job is open; the checkpoint, shard and master-finish calls
// refuse while it is on.
func (this *Context) BatchDeliveredEnable(enable bool) error {
	v := C.int(0)
	if enable {
		v = 1
	}
	return this.err(C.gdg_batch_out_records_enable(this.ctx, v))
}

// BatchDelivered: the records of the delivered rows of the last completed batch call, result[port][block] (gdg_batch_out_records).  An
// error when the call ran without them.
func (this *Context) BatchDelivered() ([][]BlockDelivered, error) {
	var ports C.int
	var blocks C.size_t
	if e := this.err(C.gdg_batch_out_records(this.ctx, nil, 0, &ports, &blocks)); e != nil {
		return nil, e
	}
	n := int(ports) * int(blocks)
	if n == 0 {
		return goBlockDelivered(nil, int(ports), int(blocks)), nil
	}
	rec := C.calloc(C.size_t(n), 40)
	if rec == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(rec)
	if e := this.err(C.gdg_batch_out_records(this.ctx, (*C.gdg_block_delivered)(rec), C.size_t(n), &ports, &blocks)); e != nil {
		return nil, e
	}
	return goBlockDelivered(rec, int(ports), int(blocks)), nil
}

// TrimFromDelivered: TrimFromTruePeak's rule on the TruePeak of the delivered rows' records (gdg_trim_from_out_records),
// records[port][block] as BatchDelivered hands them out.  Host arithmetic: no context and no device.
func TrimFromDelivered(records [][]BlockDelivered, target float64, maxGain float64) ([]float64, error) {
	ports := len(records)
	gain := make([]float64, ports)
	if ports == 0 {
		return gain, nil
	}
	blocks := len(records[0])
	for r, row := range records {
		if len(row) != blocks {
			return nil, fmt.Errorf("gdg: port %d has %d records, port 0 has %d", r, len(row), blocks)
		}
		for _, rec := range row {
			if rec.TruePeak != rec.TruePeak {
				return nil, fmt.Errorf("gdg: port %d has a NaN true peak", r)
			}
		}
	}
	rec := (*[1 << 25]C.gdg_block_delivered)(C.calloc(C.size_t(ports*blocks+1), 40))
	if rec == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(rec))
	for r, row := range records {
		for b, v := range row {
			rec[r*blocks+b].true_peak = C.double(v.TruePeak)
		}
	}
	out := (*[1 << 28]C.double)(C.calloc(C.size_t(ports), 8))
	if out == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(out))
	if rc := C.gdg_trim_from_out_records(&rec[0], C.int(ports), C.size_t(blocks), C.double(target), C.double(maxGain), &out[0]); rc != 0 {
		return nil, fmt.Errorf("gdg: gdg_trim_from_out_records: %d (target and maxGain: finite and greater than 0)", int(rc))
	}
	for i := range gain {
		gain[i] = float64(out[i])
	}
	return gain, nil
}

// ---- loudness (include/gdg.h, LOUDNESS): K-weighted hop records after ITU-R BS.1770, and the planners on them ----

// LoudnessStateDoubles: GDG_LOUDNESS_STATE_DOUBLES, what a row keeps from call to call; LoudnessTile: a continuing call begins at a multiple of it.
const (
	LoudnessStateDoubles = 7
	LoudnessTile         = 8192
)

// LoudnessCoefficients: the K-weighting at rate (gdg_loudness_coefficients): shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2.  Host arithmetic.
func LoudnessCoefficients(rate uint32) ([]float64, error) {
	out := (*[1 << 28]C.double)(C.calloc(10, 8))
	if out == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(out))
	if rc := C.gdg_loudness_coefficients(C.uint32_t(rate), &out[0]); rc != 0 {
		return nil, fmt.Errorf("gdg: gdg_loudness_coefficients: %d (rate: a multiple of 10 from 8000 on)", int(rc))
	}
	c := make([]float64, 10)
	for i := range c {
		c[i] = float64(out[i])
	}
	return c, nil
}

// LoudnessHops: the hops of rate/10 samples that complete in the job's samples [first, first+count) (gdg_loudness_hops); 0 for a rate without hops.
func LoudnessHops(rate uint32, first int, count int) int {
	return int(C.gdg_loudness_hops(C.uint32_t(rate), C.size_t(first), C.size_t(count)))
}

// LoudnessRows: rows[r] holds the samples [first, first+len) of a stream at rate (gdg_loudness_rows); result[r][h] is the sum of squares of
// the K-weighted samples of the h-th hop that completes in them.  state nil starts a stream (first must be 0); a continuing call passes
// the nRows*LoudnessStateDoubles float64 the call before returned and begins at a multiple of LoudnessTile.  Returns the records and the state.
func (this *Context) LoudnessRows(rows [][]float64, rate uint32, first int, state []float64) ([][]float64, []float64, error) {
	n := len(rows)
	if n == 0 {
		return nil, nil, fmt.Errorf("gdg: LoudnessRows needs at least one row")
	}
	count := len(rows[0])
	if state != nil && len(state) != n*LoudnessStateDoubles {
		return nil, nil, fmt.Errorf("gdg: state has %d float64, %d rows keep %d", len(state), n, n*LoudnessStateDoubles)
	}
	hops := LoudnessHops(rate, first, count)
	x := C.malloc(C.size_t(n*count*8 + 8))
	if x == nil {
		return nil, nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(x)
	for i, r := range rows {
		if len(r) != count {
			return nil, nil, fmt.Errorf("gdg: row %d has %d samples, row 0 has %d", i, len(r), count)
		}
		copy((*[1 << 37]float64)(x)[i*count:(i+1)*count:(i+1)*count], r)
	}
	st := C.calloc(C.size_t(2*n*LoudnessStateDoubles), 8)
	if st == nil {
		return nil, nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(st)
	stOut := unsafe.Pointer(uintptr(st) + uintptr(n*LoudnessStateDoubles*8))
	var stIn unsafe.Pointer
	if state != nil {
		copy((*[1 << 30]float64)(st)[:n*LoudnessStateDoubles:n*LoudnessStateDoubles], state)
		stIn = st
	}
	rec := C.calloc(C.size_t(n*hops+1), 8)
	if rec == nil {
		return nil, nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(rec)
	if e := this.err(C.gdg_loudness_rows(this.ctx, (*C.double)(x), C.size_t(count), C.int(n), C.size_t(first), C.size_t(count), C.uint32_t(rate), (*C.double)(stIn),
		(*C.double)(stOut), (*C.double)(rec), C.size_t(hops))); e != nil {
		return nil, nil, e
	}
	out := make([][]float64, n)
	for r := range out {
		out[r] = make([]float64, hops)
		copy(out[r], (*[1 << 30]float64)(rec)[r*hops:(r+1)*hops:(r+1)*hops])
	}
	next := make([]float64, n*LoudnessStateDoubles)
	copy(next, (*[1 << 30]float64)(stOut)[:n*LoudnessStateDoubles:n*LoudnessStateDoubles])
	return out, next, nil
}

// LoudnessRowsDevice: the same on device memory, enqueued on the context's stream (gdg_loudness_rows_device): row r at dRows + r*rowStride
// float64, its records at dRecords + r*recordsStride; dStateIn nil starts a stream, dStateOut may be nil or dStateIn.
func (this *Context) LoudnessRowsDevice(dRows unsafe.Pointer, rowStride int, nRows int, first int, count int, rate uint32, dStateIn unsafe.Pointer, dStateOut unsafe.Pointer,
	dRecords unsafe.Pointer, recordsStride int) error {
	return this.err(C.gdg_loudness_rows_device(this.ctx, (*C.double)(dRows), C.size_t(rowStride), C.int(nRows), C.size_t(first), C.size_t(count), C.uint32_t(rate),
		(*C.double)(dStateIn), (*C.double)(dStateOut), (*C.double)(dRecords), C.size_t(recordsStride)))
}

// BatchLoudnessEnable: from the next batch call on, BatchRun and BatchStreamStep keep the hop records of every encoded port, taken from the
// session-rate rows in front of delivery, trim and blend gain (gdg_batch_loudness_enable); off by default.  Configuration: a checkpoint does
// not carry it, an error while a streamed job is open; the checkpoint, shard and master-finish calls refuse while it is on.
func (this *Context) BatchLoudnessEnable(enable bool) error {
	v := C.int(0)
	if enable {
		v = 1
	}
	return this.err(C.gdg_batch_loudness_enable(this.ctx, v))
}

// BatchLoudness: the hop records of the last completed batch call or slice, result[port][hop] (gdg_batch_loudness).  An error when the
// call ran without them.
func (this *Context) BatchLoudness() ([][]float64, error) {
	var ports C.int
	var hops C.size_t
	if e := this.err(C.gdg_batch_loudness(this.ctx, nil, 0, &ports, &hops)); e != nil {
		return nil, e
	}
	out := make([][]float64, int(ports))
	n := int(ports) * int(hops)
	if n == 0 {
		for r := range out {
			out[r] = make([]float64, 0)
		}
		return out, nil
	}
	rec := C.calloc(C.size_t(n), 8)
	if rec == nil {
		return nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(rec)
	if e := this.err(C.gdg_batch_loudness(this.ctx, (*C.double)(rec), C.size_t(n), &ports, &hops)); e != nil {
		return nil, e
	}
	per := int(hops)
	for r := range out {
		out[r] = make([]float64, per)
		copy(out[r], (*[1 << 30]float64)(rec)[r*per:(r+1)*per:(r+1)*per])
	}
	return out, nil
}

// loudnessRecords: records[port][hop] as one C array; the caller frees it
func loudnessRecords(records [][]float64) (unsafe.Pointer, int, int, error) {
	ports := len(records)
	if ports == 0 {
		return nil, 0, 0, fmt.Errorf("gdg: no port")
	}
	hops := len(records[0])
	rec := C.calloc(C.size_t(ports*hops+1), 8)
	if rec == nil {
		return nil, 0, 0, fmt.Errorf("gdg: out of memory")
	}
	for r, row := range records {
		if len(row) != hops {
			C.free(rec)
			return nil, 0, 0, fmt.Errorf("gdg: port %d has %d hops, port 0 has %d", r, len(row), hops)
		}
		copy((*[1 << 30]float64)(rec)[r*hops:(r+1)*hops:(r+1)*hops], row)
	}
	return rec, ports, hops, nil
}

// LoudnessFromHops: the programme made of the listed ports of records[port][hop] with BS.1770's channel weights (nil: every one 1.0)
// (gdg_loudness_from_hops): integrated, largest momentary and largest short-term loudness in LUFS; -Inf where no block passes the absolute
// gate.  Host arithmetic: no context and no device.
func LoudnessFromHops(records [][]float64, rate uint32, port []int, weight []float64) (float64, float64, float64, error) {
	if len(port) == 0 || (weight != nil && len(weight) != len(port)) {
		return 0, 0, 0, fmt.Errorf("gdg: LoudnessFromHops needs at least one port, and one weight per port or none")
	}
	rec, ports, hops, e := loudnessRecords(records)
	if e != nil {
		return 0, 0, 0, e
	}
	defer C.free(rec)
	pp := (*[1 << 28]C.int)(C.calloc(C.size_t(len(port)), 4))
	if pp == nil {
		return 0, 0, 0, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(pp))
	for i, v := range port {
		pp[i] = C.int(v)
	}
	wp := (*[1 << 28]C.double)(C.calloc(C.size_t(len(port)), 8))
	if wp == nil {
		return 0, 0, 0, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(wp))
	for i := range port {
		wp[i] = 1.0
		if weight != nil {
			wp[i] = C.double(weight[i])
		}
	}
	var integrated, momentary, shortTerm C.double
	if rc := C.gdg_loudness_from_hops((*C.double)(rec), C.int(ports), C.size_t(hops), C.uint32_t(rate), &pp[0], &wp[0], C.int(len(port)), &integrated, &momentary,
		&shortTerm); rc != 0 {
		return 0, 0, 0, fmt.Errorf("gdg: gdg_loudness_from_hops: %d (%s)", int(rc), C.GoString(C.gdg_last_error(nil)))
	}
	return float64(integrated), float64(momentary), float64(shortTerm), nil
}

// TrimFromLoudness: one gain per port toward targetLufs from records[port][hop] (gdg_trim_from_loudness); with truePeak[port][block] (nil:
// no cap) a gain that would carry the port's largest true peak over ceilingDbtp is capped, and capped[port] says so.  Host arithmetic.
func TrimFromLoudness(records [][]float64, rate uint32, targetLufs float64, ceilingDbtp float64, truePeak [][]BlockTruePeak) ([]float64, []bool, error) {
	rec, ports, hops, e := loudnessRecords(records)
	if e != nil {
		return nil, nil, e
	}
	defer C.free(rec)
	blocks := 0
	var tp *C.gdg_block_true_peak
	if truePeak != nil {
		if len(truePeak) != ports {
			return nil, nil, fmt.Errorf("gdg: %d ports of true-peak records for %d ports of hop records", len(truePeak), ports)
		}
		blocks = len(truePeak[0])
		arr := (*[1 << 25]C.gdg_block_true_peak)(C.calloc(C.size_t(ports*blocks+1), 16))
		if arr == nil {
			return nil, nil, fmt.Errorf("gdg: out of memory")
		}
		defer C.free(unsafe.Pointer(arr))
		for r, row := range truePeak {
			if len(row) != blocks {
				return nil, nil, fmt.Errorf("gdg: port %d has %d true-peak records, port 0 has %d", r, len(row), blocks)
			}
			for b, v := range row {
				arr[r*blocks+b].true_peak = C.double(v.TruePeak)
			}
		}
		tp = &arr[0]
	}
	out := (*[1 << 28]C.double)(C.calloc(C.size_t(ports), 8))
	if out == nil {
		return nil, nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(out))
	cp := (*[1 << 28]C.int)(C.calloc(C.size_t(ports), 4))
	if cp == nil {
		return nil, nil, fmt.Errorf("gdg: out of memory")
	}
	defer C.free(unsafe.Pointer(cp))
	if rc := C.gdg_trim_from_loudness((*C.double)(rec), C.int(ports), C.size_t(hops), C.uint32_t(rate), C.double(targetLufs), C.double(ceilingDbtp), tp, C.size_t(blocks),
		&out[0], &cp[0]); rc != 0 {
		return nil, nil, fmt.Errorf("gdg: gdg_trim_from_loudness: %d (%s)", int(rc), C.GoString(C.gdg_last_error(nil)))
	}
	gain, capped := make([]float64, ports), make([]bool, ports)
	for i := range gain {
		gain[i] = float64(out[i])
		capped[i] = cp[i] != 0
	}
	return gain, capped, nil
}
