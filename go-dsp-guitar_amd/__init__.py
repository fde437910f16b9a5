"""go-dsp-guitar's batch-mode effects pipeline on MI355X: Python plumbing over libgdg.so.

The product is the C-ABI shared library (include/gdg.h, csrc/*.hip); this module only loads
it with ctypes and offers thin conveniences for tests and bench.py.  There is no CPU compute
path here: if the library or a GPU is missing, calls fail loudly.

The directory name contains a hyphen (it mirrors the reference's repo name), so import it
through __graft_entry__.load_package() which registers it as `go_dsp_guitar_amd`.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libgdg.so")
CSRC = os.path.join(_HERE, "csrc")

GDG_OK, GDG_ERR_INVALID, GDG_ERR_UNSUPPORTED, GDG_ERR_HIP, GDG_ERR_NO_DEVICE, GDG_ERR_NOMEM = 0, -1, -2, -3, -4, -5

UNIT_NAMES = [
    "signal_generator", "noise_gate", "bandpass", "auto_wah", "auto_yoy", "compressor", "octaver",
    "excess", "fuzz", "overdrive", "distortion", "tone_stack", "chorus", "flanger", "phaser",
    "tremolo", "ring_modulator", "delay", "reverb", "power_amp", "cabinet",
]
UNIT = {name: i for i, name in enumerate(UNIT_NAMES)}

K_FIR_FWD, K_FIR_MAC, K_FIR_INV, K_SEGMENT, K_TUNER, K_SPATIALIZER, K_WAVE, K_RESAMPLE, K_METER, K_FIR_MAC_CHAIN, K_FIR_AHEAD = range(11)
WAVE_FORMATS = {"lpcm8": 0, "lpcm16": 1, "lpcm24": 2, "lpcm32": 3, "ieee32": 4, "ieee64": 5}     # enum gdg_wave_format
KERNEL_KINDS = ["fir_fwd", "fir_mac", "fir_inv", "segment", "tuner", "spatializer"]

# every symbol include/gdg.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "gdg_version", "gdg_device_count", "gdg_ctx_create", "gdg_ctx_destroy", "gdg_last_error", "gdg_ctx_channels",
    "gdg_ctx_stream", "gdg_ctx_synchronize", "gdg_ctx_share_ir_spectra", "gdg_unit_create", "gdg_unit_destroy", "gdg_unit_set_param",
    "gdg_unit_get_param", "gdg_unit_set_fir", "gdg_unit_compile_fir", "gdg_unit_get_fir", "gdg_unit_reset", "gdg_chain_set", "gdg_process", "gdg_process_subset", "gdg_process_device",
    "gdg_staging_buffers", "gdg_process_staged", "gdg_device_alloc", "gdg_device_free", "gdg_copy_to_device", "gdg_copy_to_host", "gdg_copy_rows_device", "gdg_fft_real", "gdg_fft_real_inverse", "gdg_debug_oversample_decimate", "gdg_profile_enable",
    "gdg_profile_read", "gdg_tuner_enqueue", "gdg_tuner_enqueue_device", "gdg_tuner_enqueue_staged", "gdg_tuner_analyze", "gdg_tuner_note_name",
    "gdg_spatializer_set_position", "gdg_spatializer_set_sample_rate", "gdg_spatialize", "gdg_spatialize_device", "gdg_spatialize_staged",
    "gdg_wave_bytes_per_sample", "gdg_wave_decode", "gdg_wave_decode_device", "gdg_wave_encode", "gdg_wave_encode_device",
    "gdg_resample_time_length", "gdg_resample_time", "gdg_resample_time_device",
    "gdg_meter_configure", "gdg_meter_set_enabled", "gdg_meter_process", "gdg_meter_process_device", "gdg_meter_analyze", "gdg_meter_state",
    "gdg_metronome_set_tick", "gdg_metronome_set_tock", "gdg_metronome_configure", "gdg_metronome_process", "gdg_metronome_process_device",
    "gdg_batch_length", "gdg_batch_run", "gdg_batch_run_shard", "gdg_batch_finish_master", "gdg_batch_release", "gdg_batch_stream_span", "gdg_batch_stream_open", "gdg_batch_stream_need", "gdg_batch_stream_step", "gdg_batch_stream_close", "gdg_batch_stream_open_shard", "gdg_batch_stream_step_shard", "gdg_batch_finish_master_slice", "gdg_profile_sample", "gdg_ctx_set_window", "gdg_process_window_device", "gdg_ctx_set_overlap",
    "gdg_ctx_set_option", "gdg_ctx_get_option", "gdg_option_count", "gdg_option_name", "gdg_numa_probe", "gdg_ctx_trim", "gdg_tuner_replace",
    "gdg_state_size", "gdg_state_save", "gdg_state_save_device", "gdg_state_load", "gdg_state_load_device",
    "gdg_batch_stream_checkpoint_size", "gdg_batch_stream_checkpoint", "gdg_batch_stream_resume", "gdg_batch_stream_resume_shard", "gdg_state_verify",
    "gdg_block_stats_rows", "gdg_block_stats_rows_device", "gdg_batch_report_enable", "gdg_batch_report", "gdg_batch_set_sources",
    "gdg_batch_set_dither", "gdg_batch_dither_seek", "gdg_wave_encode_dither", "gdg_wave_encode_dither_device",
    "gdg_block_spectrum_rows", "gdg_block_spectrum_rows_device", "gdg_batch_spectrum_enable", "gdg_batch_spectrum",
    "gdg_block_align_rows", "gdg_block_align_rows_device", "gdg_batch_align_enable", "gdg_batch_align",
    "gdg_true_peak_taps", "gdg_block_true_peak_rows", "gdg_block_true_peak_rows_device", "gdg_batch_true_peak_enable", "gdg_batch_true_peak",
    "gdg_batch_set_trim", "gdg_wave_encode_trim", "gdg_wave_encode_trim_device", "gdg_trim_from_true_peak",
    "gdg_batch_set_blends", "gdg_batch_blends", "gdg_blend_rows", "gdg_blend_rows_device",
    "gdg_batch_set_blends_delayed", "gdg_batch_blend_max_delay", "gdg_blend_rows_delayed", "gdg_blend_rows_delayed_device", "gdg_blend_delays_from_align",
    "gdg_batch_set_blends_filtered", "gdg_batch_blend_max_reach", "gdg_blend_rows_filtered", "gdg_blend_rows_filtered_device", "gdg_blend_fraction_taps",
    "gdg_blend_fractions_from_fit",
    "gdg_batch_fit_enable", "gdg_batch_fits", "gdg_batch_fit", "gdg_block_fit_rows", "gdg_block_fit_rows_device", "gdg_blend_weights_from_fit",
    "gdg_batch_gram_enable", "gdg_batch_gram_ports", "gdg_batch_gram", "gdg_block_gram_rows", "gdg_block_gram_rows_device", "gdg_blend_pick_from_gram",
    "gdg_batch_tapfit_enable", "gdg_batch_tapfits", "gdg_batch_tapfit", "gdg_block_tapfit_rows", "gdg_block_tapfit_rows_device", "gdg_tapfit_doubles",
    "gdg_blend_taps_from_tapfit",
    "gdg_batch_transfer_enable", "gdg_batch_transfers", "gdg_batch_transfer", "gdg_block_transfer_rows", "gdg_block_transfer_rows_device", "gdg_transfer_doubles",
    "gdg_match_taps_from_transfer",
    "gdg_batch_set_delivery", "gdg_batch_delivery", "gdg_batch_delivery_latency", "gdg_deliver_rows", "gdg_deliver_rows_device", "gdg_deliver_taps",
    "gdg_batch_set_out_ratio", "gdg_batch_out_ratio", "gdg_batch_out_samples", "gdg_batch_out_ratio_latency", "gdg_out_ratio_taps",
    "gdg_out_ratio_rows", "gdg_out_ratio_rows_device",
    "gdg_block_out_rows", "gdg_block_out_rows_device", "gdg_batch_out_records_enable", "gdg_batch_out_records", "gdg_trim_from_out_records",
    "gdg_loudness_coefficients", "gdg_loudness_hops", "gdg_loudness_rows", "gdg_loudness_rows_device", "gdg_batch_loudness_enable", "gdg_batch_loudness",
    "gdg_loudness_from_hops", "gdg_trim_from_loudness",
]

# gdg_block_stats (include/gdg.h): one record of the render report, 32 bytes, little-endian, no padding
BLOCK_STATS_DTYPE = np.dtype([("peak", "<f8"), ("sum_sq", "<f8"), ("peak_index", "<u4"), ("clipped", "<u4"), ("full_scale", "<u4"),
                              ("nonfinite", "<u4")])
assert BLOCK_STATS_DTYPE.itemsize == 32

# gdg_block_align (include/gdg.h): one record of the alignment report, 40 bytes, little-endian
BLOCK_ALIGN_DTYPE = np.dtype([("corr", "<f8"), ("corr0", "<f8"), ("ref_sq", "<f8"), ("sq_at_lag", "<f8"), ("lag", "<i4"), ("reserved", "<u4")])
assert BLOCK_ALIGN_DTYPE.itemsize == 40
# gdg_block_true_peak (include/gdg.h): one true-peak record, 16 bytes, little-endian, no padding
BLOCK_TRUE_PEAK_DTYPE = np.dtype([("true_peak", "<f8"), ("position", "<u4"), ("overs", "<u4")])
assert BLOCK_TRUE_PEAK_DTYPE.itemsize == 16
TRUE_PEAK_BLOCK = 8192       # the true-peak record's block (include/gdg.h)


def true_peak_taps():
    """gdg_true_peak_taps: the library's [3][24] float64 interpolation taps (phases 1, 2, 3; j = -11 .. 12); no context, no device"""
    out = np.zeros((3, 24), dtype=np.float64)
    rc = lib().gdg_true_peak_taps(out.ctypes.data, out.size)
    if rc != GDG_OK:
        raise GdgError(rc, "gdg_true_peak_taps")
    return out


def trim_from_true_peak(records, target, max_gain):
    """gdg_trim_from_true_peak: the gain of every port from its true-peak records ([ports, blocks], BLOCK_TRUE_PEAK_DTYPE, as batch_true_peak
    hands them out) -- 1.0 for a silent port, else min(target / the port's largest true_peak, max_gain).  Host arithmetic: no context, no
    device.  GdgError for a NaN record (the message names the port) or a target / max_gain that is not finite and positive."""
    rec = np.ascontiguousarray(records, dtype=BLOCK_TRUE_PEAK_DTYPE)
    if rec.ndim != 2:
        raise ValueError("records: [ports, blocks]")
    gain = np.zeros(rec.shape[0], dtype=np.float64)
    rc = lib().gdg_trim_from_true_peak(rec.ctypes.data if rec.size else None, rec.shape[0], rec.shape[1], float(target), float(max_gain),
                                       gain.ctypes.data if gain.size else None)
    if rc != GDG_OK:
        raise GdgError(rc, lib().gdg_last_error(None).decode())
    return gain


# gdg_block_delivered (include/gdg.h, DELIVERED RECORDS): one record of a delivered block, 40 bytes, little-endian, no padding
BLOCK_DELIVERED_DTYPE = np.dtype([("true_peak", "<f8"), ("peak", "<f8"), ("sum_sq", "<f8"), ("position", "<i4"), ("peak_index", "<u4"), ("overs", "<u4"), ("clipped", "<u4")])
assert BLOCK_DELIVERED_DTYPE.itemsize == 40
DELIVERED_HISTORY = 23       # GDG_OUT_RECORDS_HISTORY: the samples in front of a block its record reads
DELIVERED_MAX_BLOCK = 16384  # GDG_OUT_RECORDS_MAX_BLOCK: the longest block of the stand-alone call


def trim_from_delivered(records, target, max_gain):
    """gdg_trim_from_out_records: trim_from_true_peak's rule on the true_peak of the delivered rows' records ([ports, blocks],
    BLOCK_DELIVERED_DTYPE, as batch_delivered hands them out).  Host arithmetic: no context, no device."""
    rec = np.ascontiguousarray(records, dtype=BLOCK_DELIVERED_DTYPE)
    if rec.ndim != 2:
        raise ValueError("records: [ports, blocks]")
    gain = np.zeros(rec.shape[0], dtype=np.float64)
    rc = lib().gdg_trim_from_out_records(rec.ctypes.data if rec.size else None, rec.shape[0], rec.shape[1], float(target), float(max_gain),
                                         gain.ctypes.data if gain.size else None)
    if rc != GDG_OK:
        raise GdgError(rc, lib().gdg_last_error(None).decode())
    return gain


LOUDNESS_STATE_DOUBLES = 7   # GDG_LOUDNESS_STATE_DOUBLES (include/gdg.h, LOUDNESS): what a port keeps from call to call
LOUDNESS_TILE = 8192         # GDG_LOUDNESS_TILE: a continuing call begins at a multiple of it


def loudness_coefficients(rate):
    """gdg_loudness_coefficients: the K-weighting at `rate` -- shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2; host arithmetic"""
    out = np.zeros(10, dtype=np.float64)
    rc = lib().gdg_loudness_coefficients(int(rate), out.ctypes.data)
    if rc != GDG_OK:
        raise GdgError(rc, lib().gdg_last_error(None).decode())
    return out


def loudness_hops(rate, first, count):
    """gdg_loudness_hops: the hops of rate / 10 samples that complete in the job's samples [first, first + count); 0 for a rate without hops"""
    return int(lib().gdg_loudness_hops(int(rate), int(first), int(count)))


def loudness_from_hops(records, rate, ports, weights=None):
    """gdg_loudness_from_hops: records [ports, hops] float64 (hop sums, as batch_loudness and loudness_rows hand them out); the programme is the
    listed `ports` with BS.1770's channel `weights` (None: every one 1.0).  Returns (integrated, momentary_max, short_term_max) in LUFS, -inf
    where no block passes the absolute gate.  Host arithmetic: no context, no device."""
    rec = np.ascontiguousarray(records, dtype=np.float64)
    if rec.ndim != 2:
        raise ValueError("records: [ports, hops]")
    port = np.ascontiguousarray(ports, dtype=np.int32).reshape(-1)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
    if w is not None and w.size != port.size:
        raise ValueError("one weight per listed port")
    out = [C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)]
    rc = lib().gdg_loudness_from_hops(rec.ctypes.data if rec.size else None, rec.shape[0], rec.shape[1], int(rate), port.ctypes.data if port.size else None,
                                      None if w is None else w.ctypes.data, port.size, C.byref(out[0]), C.byref(out[1]), C.byref(out[2]))
    if rc != GDG_OK:
        raise GdgError(rc, lib().gdg_last_error(None).decode())
    return tuple(v.value for v in out)


def trim_from_loudness(records, rate, target_lufs, ceiling_dbtp=0.0, true_peak=None):
    """gdg_trim_from_loudness: one gain per port toward target_lufs from its hop records [ports, hops]; with true-peak records ([ports, blocks],
    BLOCK_TRUE_PEAK_DTYPE) a gain that would carry the port over ceiling_dbtp is capped.  Returns (gain, capped).  Host arithmetic."""
    rec = np.ascontiguousarray(records, dtype=np.float64)
    if rec.ndim != 2:
        raise ValueError("records: [ports, hops]")
    tp = None if true_peak is None else np.ascontiguousarray(true_peak, dtype=BLOCK_TRUE_PEAK_DTYPE)
    if tp is not None and (tp.ndim != 2 or tp.shape[0] != rec.shape[0]):
        raise ValueError("true_peak: [ports, blocks] for the same ports")
    gain, capped = np.zeros(rec.shape[0], dtype=np.float64), np.zeros(rec.shape[0], dtype=np.int32)
    rc = lib().gdg_trim_from_loudness(rec.ctypes.data if rec.size else None, rec.shape[0], rec.shape[1], int(rate), float(target_lufs), float(ceiling_dbtp),
                                      tp.ctypes.data if tp is not None and tp.size else None, 0 if tp is None else tp.shape[1],
                                      gain.ctypes.data if gain.size else None, capped.ctypes.data if capped.size else None)
    if rc != GDG_OK:
        raise GdgError(rc, lib().gdg_last_error(None).decode())
    return gain, capped.astype(bool)


BLEND_MAX_DELAY = 4096       # GDG_BLEND_MAX_DELAY (include/gdg.h): the largest delay of a blend's term, and the samples of history a row keeps


def blend_delays_from_align(records, ref, blends, min_coeff=0.5):
    """gdg_blend_delays_from_align: records [ports, blocks] (BLOCK_ALIGN_DTYPE, as batch_align hands them out) measured with the reference
    list `ref`; blends = lists of terms whose first entry names a port (what follows it in a term is ignored).  Returns (delays, signs):
    per blend one list of ints per term -- delay_k = the blend's largest lag - the term's lag, sign_k = +1 or -1, to be multiplied into the
    weight.  Host arithmetic: no context, no device.  GdgError when a blend's terms do not share one reference port."""
    rec = np.ascontiguousarray(records, dtype=BLOCK_ALIGN_DTYPE)
    if rec.ndim != 2:
        raise ValueError("records: [ports, blocks]")
    refs = np.ascontiguousarray(np.array(ref, dtype=np.int64).reshape(-1), dtype=np.int32)
    if refs.size != rec.shape[0]:
        raise ValueError("%d references for %d ports" % (refs.size, rec.shape[0]))
    blends = [list(b) for b in blends]
    first = np.zeros(len(blends) + 1, dtype=np.int32)
    first[1:] = np.cumsum([len(b) for b in blends], dtype=np.int64)
    channel = np.array([int(t[0]) for b in blends for t in b] + [0], dtype=np.int32)
    delay, sign = np.zeros(channel.size, dtype=np.int32), np.zeros(channel.size, dtype=np.int32)
    rc = lib().gdg_blend_delays_from_align(rec.ctypes.data if rec.size else None, rec.shape[0], rec.shape[1], refs.ctypes.data if refs.size else None,
                                           float(min_coeff), len(blends), first.ctypes.data, channel.ctypes.data, delay.ctypes.data, sign.ctypes.data)
    if rc != GDG_OK:
        raise GdgError(rc, lib().gdg_last_error(None).decode())
    cut = lambda v: [[int(x) for x in v[first[b]:first[b + 1]]] for b in range(len(blends))]
    return cut(delay), cut(sign)


FIT_MAX_TERMS = 8            # GDG_FIT_MAX_TERMS (include/gdg.h): the terms of one fit
FIT_MAX_FITS = 256           # GDG_FIT_MAX_FITS: the fits of one list
FIT_BLOCK = 8192             # the block of a batch call's fit records
# gdg_block_fit (include/gdg.h): one record of the blend fit, 368 bytes, little-endian, no padding
FIT_DTYPE = np.dtype([("tt", "<f8"), ("tx", "<f8", (8,)), ("xx", "<f8", (36,)), ("skipped", "<u4"), ("terms", "<u4")])
assert FIT_DTYPE.itemsize == 368


def _fit_csr(fits):
    """fits = [(target, [ports]), ...] -> first, port, target as int32 arrays, one spare entry behind each so that an empty list has an address"""
    fits = [(int(t), [int(p) for p in ports]) for t, ports in fits]
    first = np.zeros(len(fits) + 1, dtype=np.int32)
    first[1:] = np.cumsum([len(ports) for _, ports in fits], dtype=np.int64)
    port = np.array([p for _, ports in fits for p in ports] + [0], dtype=np.int32)
    target = np.array([t for t, _ in fits] + [0], dtype=np.int32)
    return first, port, target


def blend_weights_from_fit(records, ridge=0.0):
    """gdg_blend_weights_from_fit: records [fits, blocks] (FIT_DTYPE, as batch_fit hands them out) -> (weights [fits, 8] float64, residuals
    [fits] float64): per fit the least-squares weights of its terms against its target -- (G + ridge * mean(diag G) * I) w = b, unpivoted
    Cholesky in term order -- and the share of the target's energy the fitted blend leaves.  Host arithmetic: no context, no device.
    GdgError for a silent term or a port used twice with ridge = 0 (the message names the fit)."""
    rec = np.ascontiguousarray(records, dtype=FIT_DTYPE)
    if rec.ndim != 2:
        raise ValueError("records: [fits, blocks]")
    weight = np.zeros((rec.shape[0], FIT_MAX_TERMS), dtype=np.float64)
    residual = np.zeros(rec.shape[0], dtype=np.float64)
    rc = lib().gdg_blend_weights_from_fit(rec.ctypes.data if rec.size else None, rec.shape[0], rec.shape[1], float(ridge),
                                          weight.ctypes.data if weight.size else None, residual.ctypes.data if residual.size else None)
    if rc != GDG_OK:
        raise GdgError(rc, lib().gdg_last_error(None).decode())
    return weight, residual


BLEND_MAX_TAPS = 64          # GDG_BLEND_MAX_TAPS (include/gdg.h, FILTERS): the taps of one blend term


def blend_fraction_taps(n_taps, fraction):
    """gdg_blend_fraction_taps: n_taps (even, 2 to BLEND_MAX_TAPS) windowed-sinc taps that delay by n_taps / 2 - 1 + fraction samples,
    0 <= fraction < 1, normalised to sum 1; fraction 0 is the exact unit impulse.  Host arithmetic: no context, no device."""
    tap = np.zeros(max(int(n_taps), 1), dtype=np.float64)
    rc = lib().gdg_blend_fraction_taps(int(n_taps), float(fraction), tap.ctypes.data if 2 <= int(n_taps) <= BLEND_MAX_TAPS else None)
    if rc != GDG_OK:
        raise GdgError(rc, lib().gdg_last_error(None).decode())
    return tap


def blend_fractions_from_fit(records, steps):
    """gdg_blend_fractions_from_fit: records [fits, blocks] (FIT_DTYPE) of fits whose 2 * steps - 1 terms are one channel's candidates at
    (k - (steps - 1)) / steps samples around its whole-sample plan -> one int per fit, the winner's k - (steps - 1): the candidate with the
    largest tx / sqrt(xx) over all blocks.  Host arithmetic: no context, no device.  GdgError names a fit with another term count or a
    sum that is not finite."""
    rec = np.ascontiguousarray(records, dtype=FIT_DTYPE)
    if rec.ndim != 2:
        raise ValueError("records: [fits, blocks]")
    step = np.zeros(max(rec.shape[0], 1), dtype=np.int32)
    rc = lib().gdg_blend_fractions_from_fit(rec.ctypes.data if rec.size else None, rec.shape[0], rec.shape[1], int(steps), step.ctypes.data)
    if rc != GDG_OK:
        raise GdgError(rc, lib().gdg_last_error(None).decode())
    return [int(v) for v in step[:rec.shape[0]]]


GRAM_MAX_PORTS = 512         # GDG_GRAM_MAX_PORTS (include/gdg.h): the ports of the one Gram list
GRAM_BLOCK = 8192            # the block of a batch call's Gram records


def gram_index(i, j):
    """the place of entry (i, j) in a Gram record: the lower triangle by rows (either order of i and j)"""
    i, j = (i, j) if i >= j else (j, i)
    return i * (i + 1) // 2 + j


def gram_matrix(record, n_ports):
    """one Gram record (or a sum of records), P (P + 1) / 2 doubles, as the full symmetric [P, P] matrix"""
    G = np.zeros((n_ports, n_ports), dtype=np.float64)
    G[np.tril_indices(n_ports)] = np.asarray(record, dtype=np.float64).reshape(-1)
    return G + np.tril(G, -1).T


def blend_pick_from_gram(records, n_ports, target, candidates, max_terms, ridge=0.0, min_gain=0.0):
    """gdg_blend_pick_from_gram: records [blocks, P (P + 1) / 2] float64 (as batch_gram hands them out); target and candidates are positions
    in the Gram list -> (picked, weights, residuals): the list positions picked greedily, in pick order, their least-squares weights
    against the target, and the share of the target's energy left after every pick.  Host arithmetic: no context, no device.  GdgError
    for a silent target, a NaN or inf entry, a repeated candidate or max_terms outside 1 to 8."""
    rec = np.ascontiguousarray(records, dtype=np.float64)
    if rec.ndim != 2 or rec.shape[1] != int(n_ports) * (int(n_ports) + 1) // 2:
        raise ValueError("records: [blocks, n_ports (n_ports + 1) / 2]")
    cand = np.array([int(c) for c in candidates] + [0], dtype=np.int32)
    picked = np.full(FIT_MAX_TERMS, -1, dtype=np.int32)
    weight = np.zeros(FIT_MAX_TERMS, dtype=np.float64)
    residual = np.zeros(FIT_MAX_TERMS, dtype=np.float64)
    n = C.c_int(0)
    rc = lib().gdg_blend_pick_from_gram(rec.ctypes.data if rec.size else None, int(n_ports), rec.shape[0], int(target), cand.ctypes.data, cand.size - 1, int(max_terms),
                                        float(ridge), float(min_gain), picked.ctypes.data, weight.ctypes.data, residual.ctypes.data, C.byref(n))
    if rc != GDG_OK:
        raise GdgError(rc, lib().gdg_last_error(None).decode())
    return [int(p) for p in picked[:n.value]], weight[:n.value].copy(), residual[:n.value].copy()


TAPFIT_MAX_TERMS = 4         # GDG_TAPFIT_MAX_TERMS (include/gdg.h, TAPFIT): the terms of one tap fit
TAPFIT_MAX_UNKNOWNS = 128    # GDG_TAPFIT_MAX_UNKNOWNS: terms x taps of one tap fit
TAPFIT_MAX_FITS = 16         # GDG_TAPFIT_MAX_FITS: the tap fits of one list
TAPFIT_BLOCK = 8192          # the block of a batch call's tap-fit records
TAPFIT_CHUNK = 128           # TAPFIT_KC (csrc/tapfit_kernels.h): the positions the kernel holds in LDS at a time -- no part of the record's definition


def _tapfit_csr(fits):
    """fits = [(target, [ports], taps), ...] -> first, port, target, taps as int32 arrays, one spare entry behind each"""
    fits = [(int(t), [int(p) for p in ports], int(T)) for t, ports, T in fits]
    first = np.zeros(len(fits) + 1, dtype=np.int32)
    first[1:] = np.cumsum([len(ports) for _, ports, _ in fits], dtype=np.int64)
    port = np.array([p for _, ports, _ in fits for p in ports] + [0], dtype=np.int32)
    target = np.array([t for t, _, _ in fits] + [0], dtype=np.int32)
    taps = np.array([T for _, _, T in fits] + [0], dtype=np.int32)
    return first, port, target, taps


def tapfit_doubles(fits):
    """gdg_tapfit_doubles: D, the doubles of one block's tap-fit record -- the sum over the fits of V (V + 1) / 2, V = terms x taps + 1"""
    fits = list(fits)
    first, _, _, taps = _tapfit_csr(fits)
    return int(lib().gdg_tapfit_doubles(len(fits), first.ctypes.data, taps.ctypes.data))


def tapfit_matrix(record, terms, taps):
    """one fit's part of a tap-fit record (or a sum of them), V (V + 1) / 2 doubles, as the full symmetric [V, V] matrix, V = terms x taps + 1"""
    return gram_matrix(record, int(terms) * int(taps) + 1)


def blend_taps_from_tapfit(records, fits, ridge=0.0):
    """gdg_blend_taps_from_tapfit: records [blocks, D] float64 (as batch_tapfit hands them out), fits as batch_tapfit_enable takes them ->
    (taps, residuals): per fit a [terms, T] float64 array -- term by term, lag ascending: the h_k of a filtered blend term -- and the share
    of the target's energy the fitted filters leave.  (A + ridge * mean(diag A) * I) h = b, unpivoted Cholesky in virtual-row order.  Host
    arithmetic: no context, no device.  GdgError for a pivot at or below the bound (the message names fit, term and lag: a silent or
    band-limited term, a port twice -- try ridge > 0) and for a NaN or inf entry."""
    fits = list(fits)
    first, _, _, taps = _tapfit_csr(fits)
    D = tapfit_doubles(fits)
    rec = np.ascontiguousarray(records, dtype=np.float64)
    if rec.ndim != 2 or rec.shape[1] != D:
        raise ValueError("records: [blocks, %d]" % D)
    total = int(sum((first[f + 1] - first[f]) * taps[f] for f in range(len(fits))))
    tap = np.zeros(total + 1, dtype=np.float64)
    residual = np.zeros(len(fits) + 1, dtype=np.float64)
    rc = lib().gdg_blend_taps_from_tapfit(rec.ctypes.data if rec.size else None, len(fits), first.ctypes.data, taps.ctypes.data, rec.shape[0], float(ridge),
                                          tap.ctypes.data, residual.ctypes.data)
    if rc != GDG_OK:
        raise GdgError(rc, lib().gdg_last_error(None).decode())
    out, at = [], 0
    for f in range(len(fits)):
        K, T = int(first[f + 1] - first[f]), int(taps[f])
        out.append(tap[at:at + K * T].reshape(K, T).copy())
        at += K * T
    return out, residual[:len(fits)].copy()


TRANSFER_BLOCK = 8192        # GDG_TRANSFER_BLOCK (include/gdg.h, TRANSFER): the block of a transfer record = its transform
TRANSFER_MAX_PAIRS = 16      # GDG_TRANSFER_MAX_PAIRS: the (port, target) pairs of one list
TRANSFER_MAX_GROUP = 64      # GDG_TRANSFER_MAX_GROUP: the widest group of bins, D in 1, 2, 4 .. 64


def _transfer_lists(pairs):
    """pairs = [(port, target), ...] -> port, target as int32 arrays, one spare entry behind each"""
    pairs = [(int(p), int(t)) for p, t in pairs]
    return np.array([p for p, _ in pairs] + [0], dtype=np.int32), np.array([t for _, t in pairs] + [0], dtype=np.int32)


DELIVER_HISTORY = 154        # GDG_DELIVER_HISTORY (include/gdg.h, DELIVERY): the session samples a delivered port keeps from call to call
DELIVER_ATTENUATION = 0.9440608762859234


def batch_delivery_latency(factor):
    """gdg_batch_delivery_latency: the session samples a port delivered at `factor` lags the render by (0, 38, 77)."""
    return int(lib().gdg_batch_delivery_latency(int(factor)))


def deliver_taps(factor):
    """gdg_deliver_taps: the expanded anti-aliasing taps of a delivery factor (77 at 2, 155 at 4; empty otherwise)."""
    n = int(lib().gdg_deliver_taps(int(factor), None, 0))
    out = np.zeros(n, dtype=np.float64)
    if n:
        lib().gdg_deliver_taps(int(factor), out.ctypes.data, n)
    return out


DELIVER_RATIO_HISTORY = 127  # GDG_DELIVER_RATIO_HISTORY (include/gdg.h, DELIVERY): the intermediate samples the ratio stage keeps from call to call


def batch_delivery_samples(factor, up, down, first, count):
    """gdg_batch_out_samples: the delivered samples the session samples [first, first + count) produce at factor and ratio up / down
    (both multiples of factor; 0 for anything inadmissible): what an out_bytes buffer is sized with, per job and per streamed slice."""
    return int(lib().gdg_batch_out_samples(int(factor), int(up), int(down), int(first), int(count)))


def batch_delivery_ratio_latency(factor, up, down):
    """gdg_batch_out_ratio_latency: the session samples a port delivered at factor and ratio up / down lags the render by."""
    return int(lib().gdg_batch_out_ratio_latency(int(factor), int(up), int(down)))


def deliver_ratio_taps(up, down):
    """gdg_out_ratio_taps: the ratio stage's table tap[up][T] (float64), tap[p][t] = g[p + t up]; empty for an inadmissible ratio and for 1/1."""
    n = int(lib().gdg_out_ratio_taps(int(up), int(down), None, 0))
    out = np.zeros(n, dtype=np.float64)
    if n:
        lib().gdg_out_ratio_taps(int(up), int(down), out.ctypes.data, n)
    return out.reshape(int(up), n // int(up)) if n else out


def transfer_doubles(n_pairs, group):
    """gdg_transfer_doubles: the doubles of one block's transfer record, n_pairs x (4096 / group + 1) x 4; 0 for no pair or a width that is none"""
    return int(lib().gdg_transfer_doubles(int(n_pairs), int(group)))


def match_taps_from_transfer(records, n_pairs, group, n_taps, center=0, ridge=0.0):
    """gdg_match_taps_from_transfer: records [blocks, n_pairs x G x 4] float64 (as batch_transfer hands them out; any shape of that size per
    block) -> (taps [n_pairs, n_taps], coherence [n_pairs]).  Per pair H = Sxy / (Sxx + ridge * mean Sxx) over the summed blocks, the inverse
    real transform of length N' = 8192 / group, n_taps <= N' / 2 taps around `center` under a raised-cosine taper.  Host arithmetic: no
    context, no device.  GdgError for a NaN or inf entry and for a pair with no energy in its port (the message names the pair)."""
    per = transfer_doubles(n_pairs, group)
    rec = np.ascontiguousarray(records, dtype=np.float64)
    rec = rec.reshape(rec.shape[0], -1) if rec.ndim >= 1 and rec.size else rec.reshape(0, per)
    if per and rec.shape[1] != per:
        raise ValueError("records: [blocks, %d]" % per)
    tap = np.full((max(int(n_pairs), 0), max(int(n_taps), 0)), np.nan, dtype=np.float64)
    coherence = np.full(max(int(n_pairs), 0), np.nan, dtype=np.float64)
    spare = np.zeros(1, dtype=np.float64)
    rc = lib().gdg_match_taps_from_transfer(rec.ctypes.data if rec.size else None, int(n_pairs), int(group), rec.shape[0], float(ridge), int(n_taps), int(center),
                                            tap.ctypes.data if tap.size else spare.ctypes.data, coherence.ctypes.data if coherence.size else spare.ctypes.data)
    if rc != GDG_OK:
        raise GdgError(rc, lib().gdg_last_error(None).decode())
    return tap, coherence


ALIGN_BLOCK = 8192           # the alignment report's block = its transform (include/gdg.h)
ALIGN_MAX_LAG = 2048


def align_refs(ref, max_lag):
    """A reference list of the alignment report as an int32 array, refused here as gdg_batch_align_enable refuses it: every entry -1 or a
    port of the list, 1 <= max_lag <= 2048."""
    r = np.array(ref, dtype=np.int64).reshape(-1)
    if r.size < 1:
        raise ValueError("an empty reference list")
    if not 1 <= int(max_lag) <= ALIGN_MAX_LAG:
        raise ValueError("a lag range of %d; 1 to %d" % (int(max_lag), ALIGN_MAX_LAG))
    if np.any(r < -1) or np.any(r >= r.size):
        raise ValueError("a reference is -1 or a port below %d" % r.size)
    return np.ascontiguousarray(r, dtype=np.int32)


SPECTRUM_BLOCK = 8192        # the band spectrum's block = its transform (include/gdg.h)
SPECTRUM_MAX_EDGES = 33


def spectrum_edges(edges):
    """An edge list of the band spectrum as a float64 array, refused here as gdg_batch_spectrum_enable refuses it: 2 to 33 edges, finite,
    >= 0, strictly ascending."""
    e = np.array(edges, dtype=np.float64).reshape(-1)
    if e.size < 2 or e.size > SPECTRUM_MAX_EDGES:
        raise ValueError("%d edges; 2 to %d make 1 to %d bands" % (e.size, SPECTRUM_MAX_EDGES, SPECTRUM_MAX_EDGES - 1))
    if not np.all(np.isfinite(e)) or np.any(e < 0):
        raise ValueError("an edge is a finite frequency >= 0")
    if np.any(np.diff(e) <= 0):
        raise ValueError("edges ascend strictly")
    return e


def option_names():
    """The keys gdg_ctx_set_option understands."""
    return [lib().gdg_option_name(i).decode() for i in range(lib().gdg_option_count())]


def numa_probe(sysfs_root, pci_bus_id, capacity=4096):
    """(node, [cpus]) of a PCI device from sysfs (gdg_numa_probe; no device needed)."""
    node, n = C.c_int(-1), C.c_int(0)
    cpus = (C.c_int * capacity)()
    rc = lib().gdg_numa_probe(sysfs_root.encode(), pci_bus_id.encode(), C.byref(node), cpus, capacity, C.byref(n))
    if rc != GDG_OK:
        raise GdgError(rc, "gdg_numa_probe")
    return int(node.value), [int(cpus[i]) for i in range(min(capacity, n.value))]


def checkpoint_digest(payload):
    """The 128-bit digest a checkpoint container carries over its payload (include/gdg.h states the function; the device computes it in
    state.hip).  Plain Python over the bytes: for tools that inspect a container without a GPU.  -> 16 bytes (D0, D1 little-endian)."""
    M, K, M0, M1 = (1 << 64) - 1, 0x9e3779b97f4a7c15, 0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53
    payload = bytes(payload)
    if len(payload) % 16:
        raise ValueError("a payload is a whole number of 16-byte granules")
    words = np.frombuffer(payload, dtype="<u8")
    s0 = s1 = 0
    for g in range(len(words) // 2):
        t = ((int(words[2 * g]) + (g + 1) * K) * M0) & M
        u = t ^ (t >> 32)
        s = ((int(words[2 * g + 1]) ^ u) * M1) & M
        s0 = (s0 + u) & M
        s1 ^= s ^ (s >> 29)

    def fmix(x):
        x ^= x >> 33
        x = (x * M0) & M
        x ^= x >> 33
        x = (x * M1) & M
        return x ^ (x >> 33)
    d0 = fmix((s0 + K + len(words) // 2) & M)
    d1 = fmix(s1 ^ d0)
    return d0.to_bytes(8, "little") + d1.to_bytes(8, "little")


def batch_stream_span(samples_per_channel, source_rate, target_rate, out_first, out_count):
    """(first, count): the source frames of an input that the job's output samples [out_first, out_first + out_count) read
    (gdg_batch_stream_span; pure arithmetic, no device needed)."""
    first, count = C.c_size_t(0), C.c_size_t(0)
    rc = lib().gdg_batch_stream_span(samples_per_channel, source_rate, target_rate, out_first, out_count, C.byref(first), C.byref(count))
    if rc != GDG_OK:
        raise GdgError(rc, "gdg_batch_stream_span")
    return first.value, count.value


class GdgError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("gdg error %d: %s" % (code, msg))
        self.code = code


class TunerResult(C.Structure):
    _fields_ = [("frequency", C.c_double), ("note_index", C.c_int32), ("cents", C.c_int8)]


class BatchInput(C.Structure):          # gdg_batch_input
    _fields_ = [("bytes", C.c_void_p), ("samples_per_channel", C.c_size_t), ("format", C.c_int), ("sample_rate", C.c_uint32),
                ("channels", C.c_uint), ("channel", C.c_uint)]


class BatchShardOut(C.Structure):       # gdg_batch_shard_out
    _fields_ = [("master_left", C.c_void_p), ("master_right", C.c_void_p), ("metronome_bytes", C.c_void_p), ("metronome", C.c_void_p),
                ("job_samples", C.c_size_t)]


class BatchOptions(C.Structure):        # gdg_batch_options
    _fields_ = [("target_rate", C.c_uint32), ("out_format", C.c_int), ("metronome_to_master", C.c_int), ("run_meters", C.c_int),
                ("tuner_enqueue", C.c_int)]


def build(force=False):
    """Compile libgdg.so for gfx950 with hipcc (recipe: csrc/Makefile).  Works without a GPU."""
    if force:
        subprocess.check_call(["make", "-s", "-C", CSRC, "clean"])
    subprocess.check_call(["make", "-s", "-C", CSRC])
    subprocess.check_call(["make", "-s", "-C", os.path.join(_HERE, "host")])     # C++ mirror of effects.Unit / signal.Chain
    return LIB_PATH


_lib = None


def lib():
    """The loaded libgdg.so (raises if it was never built: there is no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GdgError(GDG_ERR_NO_DEVICE, "libgdg.so is not built (run __graft_entry__.build()); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        vp, i32, u32, dbl = C.c_void_p, C.c_int, C.c_uint32, C.c_double
        sig = {
            "gdg_version": (C.c_char_p, []),
            "gdg_device_count": (i32, []),
            "gdg_ctx_create": (i32, [i32, i32, i32, C.POINTER(vp)]),
            "gdg_ctx_destroy": (i32, [vp]),
            "gdg_last_error": (C.c_char_p, [vp]),
            "gdg_ctx_channels": (i32, [vp]),
            "gdg_ctx_share_ir_spectra": (i32, [vp, i32]),
            "gdg_ctx_stream": (vp, [vp]),
            "gdg_ctx_synchronize": (i32, [vp]),
            "gdg_unit_create": (i32, [vp, i32, i32, C.POINTER(i32)]),
            "gdg_unit_destroy": (i32, [vp, i32]),
            "gdg_unit_set_param": (i32, [vp, i32, i32, C.c_int32]),
            "gdg_unit_get_param": (i32, [vp, i32, i32, C.POINTER(C.c_int32)]),
            "gdg_unit_set_fir": (i32, [vp, i32, vp, i32]),
            "gdg_unit_reset": (i32, [vp, i32]),
            "gdg_unit_compile_fir": (i32, [vp, i32, i32, vp, vp, vp, vp, u32]),
            "gdg_unit_get_fir": (i32, [vp, i32, vp, i32, C.POINTER(i32)]),
            "gdg_chain_set": (i32, [vp, i32, vp, vp, i32]),
            "gdg_state_size": (i32, [vp, vp, i32, C.POINTER(C.c_size_t)]),
            "gdg_state_save": (i32, [vp, vp, i32, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
            "gdg_state_save_device": (i32, [vp, vp, i32, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
            "gdg_state_load": (i32, [vp, vp, i32, vp, C.c_size_t]),
            "gdg_state_load_device": (i32, [vp, vp, i32, vp, C.c_size_t]),
            "gdg_batch_stream_checkpoint_size": (i32, [vp, C.POINTER(C.c_size_t)]),
            "gdg_batch_stream_checkpoint": (i32, [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
            "gdg_batch_stream_resume": (i32, [vp, vp, i32, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
            "gdg_batch_stream_resume_shard": (i32, [vp, vp, i32, vp, C.c_size_t, i32, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
            "gdg_state_verify": (i32, [vp, vp, C.c_size_t]),
            "gdg_process": (i32, [vp, vp, vp, i32, u32]),
            "gdg_process_subset": (i32, [vp, vp, i32, vp, vp, i32, u32]),
            "gdg_process_device": (i32, [vp, vp, vp, i32, u32]),
            "gdg_staging_buffers": (i32, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(i32)]),
            "gdg_process_staged": (i32, [vp, vp, i32, i32, u32]),
            "gdg_device_alloc": (i32, [vp, C.c_size_t, C.POINTER(vp)]),
            "gdg_device_free": (i32, [vp, vp]),
            "gdg_copy_to_device": (i32, [vp, vp, vp, C.c_size_t]),
            "gdg_copy_to_host": (i32, [vp, vp, vp, C.c_size_t]),
            "gdg_copy_rows_device": (i32, [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.c_size_t]),
            "gdg_fft_real": (i32, [vp, vp, i32, vp]),
            "gdg_fft_real_inverse": (i32, [vp, vp, i32, vp]),
            "gdg_debug_oversample_decimate": (i32, [vp, i32, vp, i32, vp, vp, vp]),
            "gdg_profile_enable": (i32, [vp, i32]),
            "gdg_profile_read": (i32, [vp, i32, C.POINTER(dbl), C.POINTER(i32)]),
            "gdg_tuner_enqueue": (i32, [vp, vp, i32, u32]),
            "gdg_tuner_enqueue_device": (i32, [vp, vp, i32, u32]),
            "gdg_tuner_enqueue_staged": (i32, [vp, i32, u32]),
            "gdg_tuner_analyze": (i32, [vp, C.POINTER(TunerResult)]),
            "gdg_tuner_note_name": (C.c_char_p, [i32]),
            "gdg_spatializer_set_position": (i32, [vp, i32, dbl, dbl, dbl]),
            "gdg_spatializer_set_sample_rate": (i32, [vp, u32]),
            "gdg_spatialize": (i32, [vp, vp, vp, vp, i32]),
            "gdg_spatialize_device": (i32, [vp, vp, vp, i32]),
            "gdg_spatialize_staged": (i32, [vp, i32, vp, vp, i32]),
            "gdg_wave_bytes_per_sample": (i32, [i32]),
            "gdg_wave_decode": (i32, [vp, i32, vp, C.c_size_t, C.c_uint, vp]),
            "gdg_wave_decode_device": (i32, [vp, i32, vp, C.c_size_t, C.c_uint, vp]),
            "gdg_wave_encode": (i32, [vp, i32, vp, C.c_size_t, C.c_uint, vp]),
            "gdg_wave_encode_device": (i32, [vp, i32, vp, C.c_size_t, C.c_uint, vp]),
            "gdg_resample_time_length": (i32, [i32, u32, u32]),
            "gdg_resample_time": (i32, [vp, vp, i32, u32, u32, vp, i32]),
            "gdg_resample_time_device": (i32, [vp, vp, i32, u32, u32, vp, i32]),
            "gdg_meter_configure": (i32, [vp, i32]),
            "gdg_meter_set_enabled": (i32, [vp, i32, i32]),
            "gdg_meter_process": (i32, [vp, vp, i32, u32]),
            "gdg_meter_process_device": (i32, [vp, vp, C.c_size_t, i32, u32]),
            "gdg_meter_analyze": (i32, [vp, vp, vp]),
            "gdg_meter_state": (i32, [vp, i32, C.POINTER(dbl), C.POINTER(dbl), C.POINTER(C.c_uint64)]),
            "gdg_metronome_set_tick": (i32, [vp, vp, i32]),
            "gdg_metronome_set_tock": (i32, [vp, vp, i32]),
            "gdg_metronome_configure": (i32, [vp, u32, u32, u32]),
            "gdg_metronome_process": (i32, [vp, vp, i32]),
            "gdg_metronome_process_device": (i32, [vp, vp, i32]),
            "gdg_ctx_set_window": (i32, [vp, i32]),
            "gdg_ctx_set_overlap": (i32, [vp, i32]),
            "gdg_process_window_device": (i32, [vp, vp, vp, C.c_size_t, i32, u32]),
            "gdg_batch_length": (i32, [vp, vp, i32, u32, C.POINTER(C.c_size_t)]),
            "gdg_batch_run": (i32, [vp, vp, i32, vp, vp]),
            "gdg_batch_release": (i32, [vp]),
            "gdg_batch_run_shard": (i32, [vp, vp, i32, vp, vp, vp]),
            "gdg_batch_finish_master": (i32, [vp, i32, vp, vp, i32, vp, C.c_size_t, u32, i32, vp, vp]),
            "gdg_batch_stream_span": (i32, [C.c_size_t, u32, u32, C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
            "gdg_batch_stream_open": (i32, [vp, vp, i32, vp, C.POINTER(C.c_size_t)]),
            "gdg_batch_stream_need": (i32, [vp, i32, vp, vp]),
            "gdg_batch_stream_step": (i32, [vp, i32, vp, vp]),
            "gdg_batch_stream_close": (i32, [vp]),
            "gdg_batch_stream_open_shard": (i32, [vp, vp, i32, vp, C.c_size_t, i32, C.POINTER(C.c_size_t)]),
            "gdg_batch_stream_step_shard": (i32, [vp, i32, vp, vp, vp]),
            "gdg_batch_finish_master_slice": (i32, [vp, i32, vp, vp, i32, vp, C.c_size_t, u32, i32, vp, vp]),
            "gdg_block_stats_rows": (i32, [vp, vp, i32, C.c_size_t, i32, vp]),
            "gdg_block_stats_rows_device": (i32, [vp, vp, C.c_size_t, i32, C.c_size_t, i32, vp]),
            "gdg_batch_report_enable": (i32, [vp, i32]),
            "gdg_batch_set_sources": (i32, [vp, vp, i32]),
            "gdg_batch_set_dither": (i32, [vp, i32, C.c_uint64, u32]),
            "gdg_batch_dither_seek": (i32, [vp, C.c_uint64]),
            "gdg_wave_encode_dither": (i32, [vp, i32, vp, C.c_size_t, i32, C.c_uint64, u32, C.c_uint64, vp]),
            "gdg_wave_encode_dither_device": (i32, [vp, i32, vp, C.c_size_t, i32, C.c_uint64, u32, C.c_uint64, vp]),
            "gdg_batch_report": (i32, [vp, vp, C.c_size_t, C.POINTER(i32), C.POINTER(C.c_size_t)]),
            "gdg_block_spectrum_rows": (i32, [vp, vp, i32, C.c_size_t, C.c_uint32, vp, i32, vp]),
            "gdg_block_spectrum_rows_device": (i32, [vp, vp, C.c_size_t, i32, C.c_size_t, C.c_uint32, vp, i32, vp]),
            "gdg_batch_spectrum_enable": (i32, [vp, vp, i32]),
            "gdg_batch_spectrum": (i32, [vp, vp, C.c_size_t, C.POINTER(i32), C.POINTER(C.c_size_t), C.POINTER(i32)]),
            "gdg_block_align_rows": (i32, [vp, vp, i32, C.c_size_t, vp, i32, vp]),
            "gdg_block_align_rows_device": (i32, [vp, vp, C.c_size_t, i32, C.c_size_t, vp, i32, vp]),
            "gdg_batch_align_enable": (i32, [vp, vp, i32, i32]),
            "gdg_batch_align": (i32, [vp, vp, C.c_size_t, C.POINTER(i32), C.POINTER(C.c_size_t)]),
            "gdg_true_peak_taps": (i32, [vp, i32]),
            "gdg_batch_set_trim": (i32, [vp, vp, i32, C.c_double, C.c_double, C.c_double]),
            "gdg_wave_encode_trim": (i32, [vp, i32, vp, C.c_size_t, C.c_double, i32, C.c_uint64, u32, C.c_uint64, vp]),
            "gdg_wave_encode_trim_device": (i32, [vp, i32, vp, C.c_size_t, C.c_double, i32, C.c_uint64, u32, C.c_uint64, vp]),
            "gdg_trim_from_true_peak": (i32, [vp, i32, C.c_size_t, C.c_double, C.c_double, vp]),
            "gdg_batch_set_blends": (i32, [vp, i32, vp, vp, vp, vp]),
            "gdg_batch_blends": (i32, [vp]),
            "gdg_blend_rows": (i32, [vp, vp, i32, C.c_size_t, i32, vp, vp, vp, vp]),
            "gdg_blend_rows_device": (i32, [vp, vp, C.c_size_t, i32, C.c_size_t, i32, vp, vp, vp, vp, C.c_size_t]),
            "gdg_batch_set_blends_delayed": (i32, [vp, i32, vp, vp, vp, vp, vp]),
            "gdg_batch_blend_max_delay": (i32, [vp]),
            "gdg_blend_rows_delayed": (i32, [vp, vp, i32, C.c_size_t, i32, vp, vp, vp, vp, vp, vp]),
            "gdg_blend_rows_delayed_device": (i32, [vp, vp, C.c_size_t, i32, C.c_size_t, i32, vp, vp, vp, vp, vp, C.c_size_t, vp, C.c_size_t]),
            "gdg_blend_delays_from_align": (i32, [vp, i32, C.c_size_t, vp, C.c_double, i32, vp, vp, vp, vp]),
            "gdg_batch_fit_enable": (i32, [vp, i32, vp, vp, vp]),
            "gdg_batch_fits": (i32, [vp]),
            "gdg_batch_fit": (i32, [vp, vp, C.c_size_t, C.POINTER(i32), C.POINTER(C.c_size_t)]),
            "gdg_block_fit_rows": (i32, [vp, vp, i32, C.c_size_t, i32, i32, vp, vp, vp, vp]),
            "gdg_block_fit_rows_device": (i32, [vp, vp, C.c_size_t, i32, C.c_size_t, i32, i32, vp, vp, vp, vp]),
            "gdg_blend_weights_from_fit": (i32, [vp, i32, C.c_size_t, C.c_double, vp, vp]),
            "gdg_batch_set_blends_filtered": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp]),
            "gdg_batch_blend_max_reach": (i32, [vp]),
            "gdg_blend_rows_filtered": (i32, [vp, vp, i32, C.c_size_t, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
            "gdg_blend_rows_filtered_device": (i32, [vp, vp, C.c_size_t, i32, C.c_size_t, i32, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp, C.c_size_t]),
            "gdg_blend_fraction_taps": (i32, [i32, C.c_double, vp]),
            "gdg_blend_fractions_from_fit": (i32, [vp, i32, C.c_size_t, i32, vp]),
            "gdg_batch_gram_enable": (i32, [vp, vp, i32]),
            "gdg_batch_gram_ports": (i32, [vp, vp, i32]),
            "gdg_batch_gram": (i32, [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
            "gdg_block_gram_rows": (i32, [vp, vp, i32, C.c_size_t, i32, vp, i32, vp]),
            "gdg_block_gram_rows_device": (i32, [vp, vp, C.c_size_t, i32, C.c_size_t, i32, vp, i32, vp]),
            "gdg_blend_pick_from_gram": (i32, [vp, i32, C.c_size_t, i32, vp, i32, i32, C.c_double, C.c_double, vp, vp, vp, C.POINTER(i32)]),
            "gdg_batch_tapfit_enable": (i32, [vp, i32, vp, vp, vp, vp]),
            "gdg_batch_tapfits": (i32, [vp]),
            "gdg_batch_tapfit": (i32, [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
            "gdg_block_tapfit_rows": (i32, [vp, vp, i32, C.c_size_t, i32, i32, vp, vp, vp, vp, vp]),
            "gdg_block_tapfit_rows_device": (i32, [vp, vp, C.c_size_t, i32, C.c_size_t, i32, i32, vp, vp, vp, vp, vp]),
            "gdg_tapfit_doubles": (C.c_size_t, [i32, vp, vp]),
            "gdg_blend_taps_from_tapfit": (i32, [vp, i32, vp, vp, C.c_size_t, C.c_double, vp, vp]),
            "gdg_batch_transfer_enable": (i32, [vp, i32, vp, vp, i32]),
            "gdg_batch_transfers": (i32, [vp]),
            "gdg_batch_transfer": (i32, [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
            "gdg_block_transfer_rows": (i32, [vp, vp, i32, C.c_size_t, i32, vp, vp, i32, vp]),
            "gdg_block_transfer_rows_device": (i32, [vp, vp, C.c_size_t, i32, C.c_size_t, i32, vp, vp, i32, vp]),
            "gdg_transfer_doubles": (C.c_size_t, [i32, i32]),
            "gdg_match_taps_from_transfer": (i32, [vp, i32, i32, C.c_size_t, C.c_double, i32, i32, vp, vp]),
            "gdg_batch_set_delivery": (i32, [vp, i32]),
            "gdg_batch_delivery": (i32, [vp]),
            "gdg_batch_delivery_latency": (i32, [i32]),
            "gdg_deliver_rows": (i32, [vp, vp, i32, C.c_size_t, i32, vp, vp]),
            "gdg_deliver_rows_device": (i32, [vp, vp, C.c_size_t, i32, C.c_size_t, i32, vp, vp, C.c_size_t]),
            "gdg_deliver_taps": (i32, [i32, vp, i32]),
            "gdg_batch_set_out_ratio": (i32, [vp, i32, i32, i32]),
            "gdg_batch_out_ratio": (i32, [vp, vp, vp]),
            "gdg_batch_out_samples": (C.c_size_t, [i32, i32, i32, C.c_size_t, C.c_size_t]),
            "gdg_batch_out_ratio_latency": (i32, [i32, i32, i32]),
            "gdg_out_ratio_taps": (i32, [i32, i32, vp, i32]),
            "gdg_out_ratio_rows": (i32, [vp, vp, i32, C.c_size_t, i32, i32, C.c_size_t, vp, vp, C.c_size_t]),
            "gdg_out_ratio_rows_device": (i32, [vp, vp, C.c_size_t, i32, C.c_size_t, i32, i32, C.c_size_t, vp, vp, C.c_size_t]),
            "gdg_block_out_rows": (i32, [vp, vp, i32, C.c_size_t, vp, C.c_size_t, vp, vp]),
            "gdg_block_out_rows_device": (i32, [vp, vp, C.c_size_t, i32, C.c_size_t, vp, C.c_size_t, vp, vp]),
            "gdg_batch_out_records_enable": (i32, [vp, i32]),
            "gdg_batch_out_records": (i32, [vp, vp, C.c_size_t, C.POINTER(i32), C.POINTER(C.c_size_t)]),
            "gdg_trim_from_out_records": (i32, [vp, i32, C.c_size_t, C.c_double, C.c_double, vp]),
            "gdg_loudness_coefficients": (i32, [C.c_uint32, vp]),
            "gdg_loudness_hops": (C.c_size_t, [C.c_uint32, C.c_size_t, C.c_size_t]),
            "gdg_loudness_rows": (i32, [vp, vp, C.c_size_t, i32, C.c_size_t, C.c_size_t, C.c_uint32, vp, vp, vp, C.c_size_t]),
            "gdg_loudness_rows_device": (i32, [vp, vp, C.c_size_t, i32, C.c_size_t, C.c_size_t, C.c_uint32, vp, vp, vp, C.c_size_t]),
            "gdg_batch_loudness_enable": (i32, [vp, i32]),
            "gdg_batch_loudness": (i32, [vp, vp, C.c_size_t, C.POINTER(i32), C.POINTER(C.c_size_t)]),
            "gdg_loudness_from_hops": (i32, [vp, i32, C.c_size_t, C.c_uint32, vp, vp, i32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
            "gdg_trim_from_loudness": (i32, [vp, i32, C.c_size_t, C.c_uint32, C.c_double, C.c_double, vp, C.c_size_t, vp, vp]),
            "gdg_block_true_peak_rows": (i32, [vp, vp, i32, C.c_size_t, vp]),
            "gdg_block_true_peak_rows_device": (i32, [vp, vp, C.c_size_t, i32, C.c_size_t, vp]),
            "gdg_batch_true_peak_enable": (i32, [vp, i32]),
            "gdg_batch_true_peak": (i32, [vp, vp, C.c_size_t, C.POINTER(i32), C.POINTER(C.c_size_t)]),
            "gdg_profile_sample": (i32, [vp, i32]),
            "gdg_ctx_set_option": (i32, [vp, C.c_char_p, C.c_longlong]),
            "gdg_ctx_get_option": (i32, [vp, C.c_char_p, C.POINTER(C.c_longlong)]),
            "gdg_ctx_trim": (i32, [vp]),
            "gdg_tuner_replace": (i32, [vp, i32, vp, i32, u32]),
            "gdg_option_count": (i32, []),
            "gdg_option_name": (C.c_char_p, [i32]),
            "gdg_numa_probe": (i32, [C.c_char_p, C.c_char_p, C.POINTER(i32), C.POINTER(i32), i32, C.POINTER(i32)]),
        }
        for name, (res, args) in sig.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def device_count():
    return lib().gdg_device_count()


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class DeviceBuffer:
    """A [rows][cols] float64 array in the context's device memory (plain device pointer underneath)."""

    def __init__(self, ctx, rows, cols):
        self.ctx, self.rows, self.cols = ctx, rows, cols
        p = C.c_void_p()
        ctx._check(lib().gdg_device_alloc(ctx._h, rows * cols * 8, C.byref(p)))
        self.ptr = p.value

    def upload(self, a):
        a = _f64(a)
        assert a.size == self.rows * self.cols
        self.ctx._check(lib().gdg_copy_to_device(self.ctx._h, self.ptr, a.ctypes.data, a.nbytes))

    def download(self):
        out = np.empty((self.rows, self.cols), dtype=np.float64)
        self.ctx._check(lib().gdg_copy_to_host(self.ctx._h, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            lib().gdg_device_free(self.ctx._h, self.ptr)
            self.ptr = None


class Context:
    """One shard of channels on one GPU (gdg_ctx)."""

    def __init__(self, n_channels, max_frames=8192, device=0):
        self.n_channels, self.max_frames, self.device = n_channels, max_frames, device
        h = C.c_void_p()
        rc = lib().gdg_ctx_create(n_channels, max_frames, device, C.byref(h))
        if rc != GDG_OK:
            raise GdgError(rc, "gdg_ctx_create failed (no usable HIP device?)")
        self._h = h
        self._chains = [[] for _ in range(n_channels)]      # [(handle, bypass)]

    def close(self):
        if getattr(self, "_h", None):
            lib().gdg_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def share_ir_spectra(self, enable):
        self._check(lib().gdg_ctx_share_ir_spectra(self._h, 1 if enable else 0))

    def _check(self, rc):
        if rc != GDG_OK:
            raise GdgError(rc, lib().gdg_last_error(self._h).decode())

    # -- units / chains ------------------------------------------------------------------------
    def unit_create(self, channel, unit_type):
        if isinstance(unit_type, str):
            unit_type = UNIT[unit_type]
        h = C.c_int(-1)
        self._check(lib().gdg_unit_create(self._h, channel, unit_type, C.byref(h)))
        return h.value

    def unit_destroy(self, handle):
        self._check(lib().gdg_unit_destroy(self._h, handle))

    def unit_set_param(self, handle, idx, value):
        self._check(lib().gdg_unit_set_param(self._h, handle, idx, int(value)))

    def unit_get_param(self, handle, idx):
        v = C.c_int32(0)
        self._check(lib().gdg_unit_get_param(self._h, handle, idx, C.byref(v)))
        return v.value

    def unit_set_fir(self, handle, taps):
        t = _f64(taps)
        self._check(lib().gdg_unit_set_fir(self._h, handle, t.ctypes.data if t.size else None, t.size))

    def unit_compile_fir(self, handle, filters, target_order=0):
        """filters: list of (taps or None, gain_compensation_factor, level_db) per slot (gdg_unit_compile_fir)."""
        n = len(filters)
        arrs = [(_f64(t) if t is not None else None) for t, _, _ in filters]
        ptrs = (C.c_void_p * n)(*[(a.ctypes.data if a is not None and a.size else None) for a in arrs])
        lens = (C.c_int * n)(*[(a.size if a is not None else 0) for a in arrs])
        comp = (C.c_double * n)(*[float(f[1]) for f in filters])
        lev = (C.c_int32 * n)(*[int(f[2]) for f in filters])
        self._check(lib().gdg_unit_compile_fir(self._h, handle, n, ptrs, lens, comp, lev, target_order))

    def unit_get_fir(self, handle):
        n = C.c_int(0)
        self._check(lib().gdg_unit_get_fir(self._h, handle, None, 0, C.byref(n)))
        out = np.empty(n.value, dtype=np.float64)
        if n.value:
            self._check(lib().gdg_unit_get_fir(self._h, handle, out.ctypes.data, n.value, C.byref(n)))
        return out

    def unit_reset(self, handle):
        self._check(lib().gdg_unit_reset(self._h, handle))

    def chain_set(self, channel, handles, bypass=None):
        n = len(handles)
        bypass = [False] * n if bypass is None else bypass
        hs = (C.c_int * max(n, 1))(*handles)
        bs = (C.c_uint8 * max(n, 1))(*[1 if b else 0 for b in bypass])
        self._check(lib().gdg_chain_set(self._h, channel, hs, bs, n))
        self._chains[channel] = list(zip(handles, bypass))

    def append_unit(self, channel, unit_type, params=None, fir=None, bypass=False):
        """AppendUnit + SetBypass + parameter set-up in one go (test convenience)."""
        h = self.unit_create(channel, unit_type)
        if params is not None:
            for i, v in enumerate(params):
                self.unit_set_param(h, i, v)
        if fir is not None:
            self.unit_set_fir(h, fir)
        chain = self._chains[channel] + [(h, bypass)]
        self.chain_set(channel, [c[0] for c in chain], [c[1] for c in chain])
        return h

    # -- channel state (gdg_state_*): save / load what the channels carry from one call to the next ---------
    @staticmethod
    def _channels(channels):
        if channels is None:
            return None, 0
        n = len(channels)
        return (C.c_int * max(n, 1))(*channels), n

    def state_size(self, channels=None):
        chans, n = self._channels(channels)
        b = C.c_size_t(0)
        self._check(lib().gdg_state_size(self._h, chans, n, C.byref(b)))
        return b.value

    def save_state(self, channels=None):
        """-> bytes: one record per listed channel (None: all), in list order."""
        chans, n = self._channels(channels)
        size = self.state_size(channels)
        buf = C.create_string_buffer(max(size, 1))
        written = C.c_size_t(0)
        self._check(lib().gdg_state_save(self._h, chans, n, buf, size, C.byref(written)))
        return buf.raw[:written.value]

    def load_state(self, blob, channels=None):
        """Record i of `blob` into channels[i] (None: all channels in order); nothing changes when it is rejected."""
        chans, n = self._channels(channels)
        blob = bytes(blob)
        self._check(lib().gdg_state_load(self._h, chans, n, blob, len(blob)))

    def save_state_device(self, dev, channels=None, capacity=None):
        """Into a device buffer (a DeviceBuffer or a plain 16-byte-aligned device pointer with `capacity`); -> bytes written."""
        chans, n = self._channels(channels)
        ptr = dev.ptr if isinstance(dev, DeviceBuffer) else dev
        cap = dev.rows * dev.cols * 8 if isinstance(dev, DeviceBuffer) else capacity
        written = C.c_size_t(0)
        self._check(lib().gdg_state_save_device(self._h, chans, n, ptr, cap, C.byref(written)))
        return written.value

    def load_state_device(self, dev, nbytes, channels=None):
        chans, n = self._channels(channels)
        ptr = dev.ptr if isinstance(dev, DeviceBuffer) else dev
        self._check(lib().gdg_state_load_device(self._h, chans, n, ptr, nbytes))

    # -- processing --------------------------------------------------------------------------------
    def process(self, x, sample_rate):
        """x: [n_channels][frames] host array -> same-shaped output (gdg_process, blocking)."""
        x = _f64(x)
        assert x.ndim == 2 and x.shape[0] == self.n_channels
        frames = x.shape[1]
        out = np.empty_like(x)
        ins = (C.c_void_p * self.n_channels)(*[x[c].ctypes.data for c in range(self.n_channels)])
        outs = (C.c_void_p * self.n_channels)(*[out[c].ctypes.data for c in range(self.n_channels)])
        self._check(lib().gdg_process(self._h, ins, outs, frames, sample_rate))
        return out

    def process_subset(self, channels, x, sample_rate):
        """x: [len(channels)][frames]; only the listed channels' chains run (gdg_process_subset)."""
        x = _f64(x)
        n = len(channels)
        assert x.ndim == 2 and x.shape[0] == n
        out = np.empty_like(x)
        chans = (C.c_int * n)(*channels)
        ins = (C.c_void_p * n)(*[x[i].ctypes.data for i in range(n)])
        outs = (C.c_void_p * n)(*[out[i].ctypes.data for i in range(n)])
        self._check(lib().gdg_process_subset(self._h, chans, n, ins, outs, x.shape[1], sample_rate))
        return out

    def process_staged(self, channels, x, sample_rate):
        """The cgo-friendly path: copy frames into the pinned slab rows, gdg_process_staged, copy rows out."""
        x = _f64(x)
        n, frames = x.shape
        pin, pout, stride = C.c_void_p(), C.c_void_p(), C.c_int(0)
        self._check(lib().gdg_staging_buffers(self._h, C.byref(pin), C.byref(pout), C.byref(stride)))
        slab_in = np.ctypeslib.as_array(C.cast(pin, C.POINTER(C.c_double)), shape=(self.n_channels, stride.value))
        slab_out = np.ctypeslib.as_array(C.cast(pout, C.POINTER(C.c_double)), shape=(self.n_channels, stride.value))
        idx = np.asarray(channels, dtype=np.intp)
        slab_in[idx, :frames] = x
        chans = (C.c_int * n)(*channels)
        self._check(lib().gdg_process_staged(self._h, chans, n, frames, sample_rate))
        return slab_out[idx, :frames].copy()

    def process_device(self, d_in, d_out, frames, sample_rate):
        """Device-resident block; d_in / d_out are plain device pointers (ints) or DeviceBuffers."""
        pi = d_in.ptr if isinstance(d_in, DeviceBuffer) else d_in
        po = d_out.ptr if isinstance(d_out, DeviceBuffer) else d_out
        self._check(lib().gdg_process_device(self._h, pi, po, frames, sample_rate))

    def synchronize(self):
        self._check(lib().gdg_ctx_synchronize(self._h))

    def alloc(self, rows, cols):
        return DeviceBuffer(self, rows, cols)

    @property
    def stream(self):
        return lib().gdg_ctx_stream(self._h)

    # -- profiling ------------------------------------------------------------------------------------
    def profile_enable(self, on=True, kinds=None):
        """on: every kernel launch; kinds: only the listed kernel kinds (cheaper inside a timed region)."""
        mask = sum(1 << (k + 1) for k in kinds) if kinds else (1 if on else 0)
        self._check(lib().gdg_profile_enable(self._h, mask))

    def profile_sample(self, every):
        self._check(lib().gdg_profile_sample(self._h, every))

    def profile_read(self, kind):
        ms, n = C.c_double(0.0), C.c_int(0)
        self._check(lib().gdg_profile_read(self._h, kind, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    # -- the transforms underneath the power amp -------------------------------------------------------
    def fft_real(self, x):
        """fft.RealFourier: n reals -> n / 2 + 1 complex bins."""
        x = _f64(x)
        out = np.empty(2 * (x.size // 2 + 1), dtype=np.float64)
        self._check(lib().gdg_fft_real(self._h, x.ctypes.data, x.size, out.ctypes.data))
        return out.view(np.complex128)

    def debug_oversample_decimate(self, factor, x, state):
        """OversamplerDecimator.Oversample then Decimate on the HIP tiles (debug entry); `state` (8 + taps - 1 doubles, zeros = fresh) is updated in place.
        Returns (oversampled, decimated)."""
        x = _f64(x)
        assert state.dtype == np.float64 and state.flags.c_contiguous
        up, down = np.empty(factor * x.size), np.empty(x.size)
        self._check(lib().gdg_debug_oversample_decimate(self._h, factor, x.ctypes.data, x.size, state.ctypes.data, up.ctypes.data, down.ctypes.data))
        return up, down

    def fft_real_inverse(self, spectrum, n):
        s = np.ascontiguousarray(spectrum, dtype=np.complex128)
        assert s.size == n // 2 + 1
        out = np.empty(n, dtype=np.float64)
        self._check(lib().gdg_fft_real_inverse(self._h, s.ctypes.data, n, out.ctypes.data))
        return out

    # -- tuner / spatializer ---------------------------------------------------------------------------
    def tuner_enqueue(self, x, sample_rate):
        x = _f64(x)
        assert x.ndim == 2 and x.shape[0] == self.n_channels
        ptrs = (C.c_void_p * self.n_channels)(*[x[c].ctypes.data for c in range(self.n_channels)])
        self._check(lib().gdg_tuner_enqueue(self._h, ptrs, x.shape[1], sample_rate))

    def tuner_enqueue_device(self, d_x, frames, sample_rate):
        p = d_x.ptr if isinstance(d_x, DeviceBuffer) else d_x
        self._check(lib().gdg_tuner_enqueue_device(self._h, p, frames, sample_rate))

    def tuner_analyze(self, raw=False):
        """raw=True: the C structs as the call left them (what a C or Go caller gets; building 256 dicts costs Python ~0.1 ms)"""
        res = (TunerResult * self.n_channels)()
        self._check(lib().gdg_tuner_analyze(self._h, res))
        if raw:
            return res
        return [{"frequency": r.frequency, "note_index": r.note_index, "cents": r.cents,
                 "note": lib().gdg_tuner_note_name(r.note_index).decode()} for r in res]

    def spatializer_set_position(self, channel, azimuth, distance, level):
        self._check(lib().gdg_spatializer_set_position(self._h, channel, azimuth, distance, level))

    def spatializer_set_sample_rate(self, rate):
        self._check(lib().gdg_spatializer_set_sample_rate(self._h, rate))

    def spatialize(self, x):
        x = _f64(x)
        assert x.ndim == 2 and x.shape[0] == self.n_channels
        n = x.shape[1]
        ptrs = (C.c_void_p * self.n_channels)(*[x[c].ctypes.data for c in range(self.n_channels)])
        left, right = np.empty(n), np.empty(n)
        self._check(lib().gdg_spatialize(self._h, ptrs, left.ctypes.data, right.ctypes.data, n))
        return left, right

    def spatialize_device(self, d_x, d_out_lr, frames):
        pi = d_x.ptr if isinstance(d_x, DeviceBuffer) else d_x
        po = d_out_lr.ptr if isinstance(d_out_lr, DeviceBuffer) else d_out_lr
        self._check(lib().gdg_spatialize_device(self._h, pi, po, frames))

    # -- data formats either side of the path -------------------------------------------
    def wave_decode(self, fmt, data, channels=1):
        """Data section of a WAVE file (interleaved bytes) -> planar float64 [channels][n]."""
        f = WAVE_FORMATS[fmt] if isinstance(fmt, str) else fmt
        data = np.ascontiguousarray(data, dtype=np.uint8)
        w = lib().gdg_wave_bytes_per_sample(f)
        per = data.size // (w * channels) if w else 0
        out = np.empty((channels, per), dtype=np.float64)
        self._check(lib().gdg_wave_decode(self._h, f, data.ctypes.data, per, channels, out.ctypes.data))
        return out[0] if channels == 1 else out

    def wave_encode(self, fmt, samples):
        """Planar float64 [channels][n] (or [n]) -> interleaved little-endian bytes."""
        f = WAVE_FORMATS[fmt] if isinstance(fmt, str) else fmt
        x = _f64(samples)
        channels, per = (1, x.size) if x.ndim == 1 else x.shape
        out = np.empty(channels * per * max(lib().gdg_wave_bytes_per_sample(f), 1), dtype=np.uint8)
        self._check(lib().gdg_wave_encode(self._h, f, x.ctypes.data, per, channels, out.ctypes.data))
        return out

    def resample_time(self, samples, source_rate, target_rate):
        x = _f64(samples)
        n_out = lib().gdg_resample_time_length(x.size, source_rate, target_rate)
        out = np.empty(max(n_out, 0), dtype=np.float64)
        self._check(lib().gdg_resample_time(self._h, x.ctypes.data, x.size, source_rate, target_rate, out.ctypes.data, n_out))
        return out

    def meter_configure(self, n_ports):
        self._n_ports = n_ports
        self._check(lib().gdg_meter_configure(self._h, n_ports))

    def meter_set_enabled(self, enabled, port=-1):
        self._check(lib().gdg_meter_set_enabled(self._h, port, 1 if enabled else 0))

    def meter_process(self, x, sample_rate):
        x = _f64(x)
        assert x.ndim == 2 and x.shape[0] == self._n_ports
        ptrs = (C.c_void_p * self._n_ports)(*[x[p].ctypes.data for p in range(self._n_ports)])
        self._check(lib().gdg_meter_process(self._h, ptrs, x.shape[1], sample_rate))

    def meter_process_device(self, d_rows, row_stride, frames, sample_rate):
        p = d_rows.ptr if isinstance(d_rows, DeviceBuffer) else d_rows
        self._check(lib().gdg_meter_process_device(self._h, p, row_stride, frames, sample_rate))

    def meter_analyze(self):
        lv = np.empty(self._n_ports, dtype=np.int32)
        pk = np.empty(self._n_ports, dtype=np.int32)
        self._check(lib().gdg_meter_analyze(self._h, lv.ctypes.data, pk.ctypes.data))
        return lv, pk

    def meter_state(self, port):
        c, p, n = C.c_double(), C.c_double(), C.c_uint64()
        self._check(lib().gdg_meter_state(self._h, port, C.byref(c), C.byref(p), C.byref(n)))
        return c.value, p.value, n.value

    def metronome_set_sounds(self, tick, tock):
        for fn, a in ((lib().gdg_metronome_set_tick, tick), (lib().gdg_metronome_set_tock, tock)):
            if a is None:
                self._check(fn(self._h, None, 0))
            else:
                a = _f64(a)
                self._check(fn(self._h, a.ctypes.data if a.size else C.cast(C.create_string_buffer(8), C.c_void_p), a.size))

    def metronome_configure(self, beats_per_period, bpm_speed, sample_rate):
        self._check(lib().gdg_metronome_configure(self._h, beats_per_period, bpm_speed, sample_rate))

    def set_window(self, frames_per_call):
        """Time blocking: up to `frames_per_call` (1, 2, 4, 8, 16) consecutive 8192-sample frames per channel and call."""
        self._check(lib().gdg_ctx_set_window(self._h, frames_per_call))

    def tuner_replace(self, channel, samples, sample_rate):
        """One channel's whole 96000-sample ring, oldest first (gdg_tuner_replace)."""
        a = np.ascontiguousarray(samples, dtype=np.float64)
        self._check(lib().gdg_tuner_replace(self._h, channel, a.ctypes.data, a.size, sample_rate))

    def trim(self):
        """Give spare device memory back (gdg_ctx_trim); blocks."""
        self._check(lib().gdg_ctx_trim(self._h))

    def set_option(self, key, value):
        """Launch-shape options (include/gdg.h, gdg_ctx_set_option): what used to be environment variables."""
        self._check(lib().gdg_ctx_set_option(self._h, key.encode(), int(value)))

    def get_option(self, key):
        v = C.c_longlong(0)
        self._check(lib().gdg_ctx_get_option(self._h, key.encode(), C.byref(v)))
        return int(v.value)

    def set_overlap(self, groups):
        """Channel groups of the device-resident calls, free-running on streams of their own (include/gdg.h)."""
        self._check(lib().gdg_ctx_set_overlap(self._h, groups))

    def process_window_device(self, d_in, d_out, row_stride, frames_in_window, sample_rate):
        pi = d_in.ptr if isinstance(d_in, DeviceBuffer) else d_in
        po = d_out.ptr if isinstance(d_out, DeviceBuffer) else d_out
        self._check(lib().gdg_process_window_device(self._h, pi, po, row_stride, frames_in_window, sample_rate))

    def _batch_inputs(self, inputs):
        n = len(inputs)
        arr = (BatchInput * n)()
        keep = []
        for i, it in enumerate(inputs):
            if it is None:
                continue
            data, fmt, rate = it[0], it[1], it[2]
            channels, channel = (it[3], it[4]) if len(it) > 3 else (1, 0)
            f = WAVE_FORMATS[fmt] if isinstance(fmt, str) else fmt
            data = np.ascontiguousarray(data, dtype=np.uint8)
            keep.append(data)
            w = max(lib().gdg_wave_bytes_per_sample(f), 1)
            arr[i] = BatchInput(data.ctypes.data if data.size else None, data.size // (w * max(channels, 1)), f, rate, channels, channel)
        return arr, keep

    def batch_length(self, inputs, target_rate):
        arr, _keep = self._batch_inputs(inputs)
        length = C.c_size_t(0)
        self._check(lib().gdg_batch_length(self._h, arr, len(inputs), target_rate, C.byref(length)))
        return length.value

    def batch_run(self, inputs, target_rate, out_format, metronome_to_master=False, run_meters=False, tuner_enqueue=False, outs=None, skip_outputs=False):
        """controller.processFiles on the device (controller/controller.go:2809-3219 without prompts and file I/O).
        inputs: per channel None ("leaving channel empty") or (data-section bytes, format, sample_rate[, channels, channel]);
        returns the N + 3 output data sections (uint8 arrays): out_0 .. out_{N-1}, master left, master right, metronome -- and behind them
        one per blend in force (batch_set_blends).  skip_outputs: every output pointer NULL -- the job renders and measures (the records
        that are switched on), nothing is written; returns None."""
        n = len(inputs)
        no = n + 3 + self.batch_blends()
        arr, _keep = self._batch_inputs(inputs)
        fo = WAVE_FORMATS[out_format] if isinstance(out_format, str) else out_format
        opt = BatchOptions(target_rate, fo, int(bool(metronome_to_master)), int(bool(run_meters)), int(bool(tuner_enqueue)))
        length = C.c_size_t(0)
        self._check(lib().gdg_batch_length(self._h, arr, n, target_rate, C.byref(length)))
        wo = lib().gdg_wave_bytes_per_sample(fo)
        size = self._delivered(0, length.value) * wo          # every port at the delivered rate (batch_set_delivery, batch_set_delivery_ratio)
        if skip_outputs:
            self._check(lib().gdg_batch_run(self._h, arr, n, C.byref(opt), (C.c_void_p * no)()))
            return None
        if outs is None:
            outs = [np.zeros(size, dtype=np.uint8) for _ in range(no)]
        assert len(outs) == no and all(o.dtype == np.uint8 and o.size == size for o in outs)
        ptrs = (C.c_void_p * no)(*[(o.ctypes.data if o.size else None) for o in outs])
        self._check(lib().gdg_batch_run(self._h, arr, n, C.byref(opt), ptrs))
        return outs

    def batch_prepared(self, inputs, target_rate, out_format, metronome_to_master=False, run_meters=False, tuner_enqueue=False):
        """gdg_batch_run with its arguments marshalled ONCE: returns (call, outs); call() is the C call alone (what a C or Go caller pays --
        filling 512 input structs and 515 pointers in Python costs ~3 ms per run), outs the N + 3 output buffers it writes."""
        n = len(inputs)
        arr, keep = self._batch_inputs(inputs)
        fo = WAVE_FORMATS[out_format] if isinstance(out_format, str) else out_format
        opt = BatchOptions(target_rate, fo, int(bool(metronome_to_master)), int(bool(run_meters)), int(bool(tuner_enqueue)))
        length = C.c_size_t(0)
        self._check(lib().gdg_batch_length(self._h, arr, n, target_rate, C.byref(length)))
        wo = lib().gdg_wave_bytes_per_sample(fo)
        no = n + 3 + self.batch_blends()                # the blends in force when the call is prepared
        outs = [np.zeros(self._delivered(0, length.value) * wo, dtype=np.uint8) for _ in range(no)]      # ... and the delivery in force
        ptrs = (C.c_void_p * no)(*[(o.ctypes.data if o.size else None) for o in outs])
        fn, h, ref = lib().gdg_batch_run, self._h, C.byref(opt)

        def call(_keep=(keep, arr, opt, ptrs, outs)):
            self._check(fn(h, arr, n, ref, ptrs))
        return call, outs

    def batch_shard_prepared(self, inputs, target_rate, out_format, job_samples=0, metronome=False, run_meters=False, tuner_enqueue=False):
        """gdg_batch_run_shard with its arguments marshalled and its result buffers allocated ONCE: returns (call, result) where call() is the C
        call alone and result = (outs, left, right, metronome_bytes, metronome_f64) as batch_run_shard returns them."""
        n = len(inputs)
        arr, keep = self._batch_inputs(inputs)
        fo = WAVE_FORMATS[out_format] if isinstance(out_format, str) else out_format
        opt = BatchOptions(target_rate, fo, 0, int(bool(run_meters)), int(bool(tuner_enqueue)))
        length = job_samples or self.batch_length(inputs, target_rate)
        wo = lib().gdg_wave_bytes_per_sample(fo)
        outs = [np.zeros(length * wo, dtype=np.uint8) for _ in range(n)]
        left, right = np.zeros(max(length, 1)), np.zeros(max(length, 1))
        mb = np.zeros(length * wo, dtype=np.uint8) if metronome else None
        mf = np.zeros(length) if metronome else None
        ptrs = (C.c_void_p * n)(*[(o.ctypes.data if o.size else None) for o in outs])
        so = BatchShardOut(left.ctypes.data, right.ctypes.data, mb.ctypes.data if (metronome and length) else None,
                           mf.ctypes.data if (metronome and length) else None, job_samples)
        fn, h, ropt, rso = lib().gdg_batch_run_shard, self._h, C.byref(opt), C.byref(so)

        def call(_keep=(keep, arr, opt, ptrs, so, outs, left, right, mb, mf)):
            self._check(fn(h, arr, n, ropt, ptrs, rso))
        return call, (outs, left[:length], right[:length], mb, mf)

    def batch_run_shard(self, inputs, target_rate, out_format, job_samples=0, metronome=False, run_meters=False, tuner_enqueue=False, outs=None):
        """One shard of a batch split over several contexts (gdg_batch_run_shard): returns (outs, left, right, metronome_bytes,
        metronome_f64): the shard's n encoded chain outputs, its float64 partial master mix, and -- on the shard that runs the
        metronome -- the encoded metronome track and its float64 samples (the master's aux input)."""
        n = len(inputs)
        arr, _keep = self._batch_inputs(inputs)
        fo = WAVE_FORMATS[out_format] if isinstance(out_format, str) else out_format
        opt = BatchOptions(target_rate, fo, 0, int(bool(run_meters)), int(bool(tuner_enqueue)))
        length = job_samples or self.batch_length(inputs, target_rate)
        wo = lib().gdg_wave_bytes_per_sample(fo)
        if outs is None:
            outs = [np.zeros(length * wo, dtype=np.uint8) for _ in range(n)]
        left, right = np.zeros(length), np.zeros(length)
        mb = np.zeros(length * wo, dtype=np.uint8) if metronome else None
        mf = np.zeros(length) if metronome else None
        ptrs = (C.c_void_p * n)(*[(o.ctypes.data if o.size else None) for o in outs])
        so = BatchShardOut(left.ctypes.data if length else None, right.ctypes.data if length else None,
                           mb.ctypes.data if (metronome and length) else None, mf.ctypes.data if (metronome and length) else None, job_samples)
        if length == 0:
            so = BatchShardOut(left.ctypes.data_as(C.c_void_p), right.ctypes.data_as(C.c_void_p), None, None, job_samples)
        self._check(lib().gdg_batch_run_shard(self._h, arr, n, C.byref(opt), ptrs, C.byref(so)))
        return outs, left, right, mb, mf

    def batch_finish_master(self, out_format, lefts, rights, aux=None, sample_rate=0, run_meters=False):
        """master = sum of the shards' partial mixes (in shard order) + aux, encoded on this context's device."""
        G, n = len(lefts), lefts[0].size
        fo = WAVE_FORMATS[out_format] if isinstance(out_format, str) else out_format
        wo = lib().gdg_wave_bytes_per_sample(fo)
        lefts = [_f64(a) for a in lefts]
        rights = [_f64(a) for a in rights]
        lp = (C.c_void_p * G)(*[a.ctypes.data for a in lefts])
        rp = (C.c_void_p * G)(*[a.ctypes.data for a in rights])
        ml, mr = np.zeros(n * wo, dtype=np.uint8), np.zeros(n * wo, dtype=np.uint8)
        a = _f64(aux) if aux is not None else None
        self._check(lib().gdg_batch_finish_master(self._h, fo, lp, rp, G, a.ctypes.data if a is not None else None, n, sample_rate,
                                                  int(bool(run_meters)), ml.ctypes.data if n else None, mr.ctypes.data if n else None))
        return ml, mr

    # -- the streamed batch run: the job of batch_run in slices of whole blocks (gdg_batch_stream_*) --------------------------
    @staticmethod
    def _stream_metas(inputs):
        arr = (BatchInput * len(inputs))()
        for i, it in enumerate(inputs):
            if it is None or not it[0]:
                continue
            channels, channel = (it[3], it[4]) if len(it) > 3 else (1, 0)
            f = WAVE_FORMATS[it[1]] if isinstance(it[1], str) else it[1]
            arr[i] = BatchInput(C.addressof(arr), int(it[0]), f, it[2], channels, channel)      # bytes: never read, only "not NULL"
        return arr

    @staticmethod
    def _stream_split(inputs):
        """(metas, datas, widths) of batch_run's input tuples: what the open call is told, the data sections, bytes per frame"""
        metas, datas, widths = [], [], []
        for it in inputs:
            if it is None:
                metas.append(None), datas.append(None), widths.append(0)
                continue
            data = np.ascontiguousarray(it[0], dtype=np.uint8)
            f = WAVE_FORMATS[it[1]] if isinstance(it[1], str) else it[1]
            channels = it[3] if len(it) > 3 else 1
            w = max(lib().gdg_wave_bytes_per_sample(f), 1) * max(channels, 1)
            metas.append((data.size // w,) + tuple(it[1:])), datas.append(data), widths.append(w)
        return metas, datas, widths

    def batch_stream_open(self, inputs, target_rate, out_format, metronome_to_master=False, run_meters=False, tuner_enqueue=False):
        """inputs: per channel None or (samples_per_channel of the FILE, format, sample_rate[, channels, channel]); returns the samples of
        every output."""
        n = len(inputs)
        arr = self._stream_metas(inputs)
        fo = WAVE_FORMATS[out_format] if isinstance(out_format, str) else out_format
        opt = BatchOptions(target_rate, fo, int(bool(metronome_to_master)), int(bool(run_meters)), int(bool(tuner_enqueue)))
        length = C.c_size_t(0)
        self._check(lib().gdg_batch_stream_open(self._h, arr, n, C.byref(opt), C.byref(length)))
        self._stream_width = lib().gdg_wave_bytes_per_sample(fo)
        self._stream_done = 0                           # session samples of the slices so far: what a ratio counts a slice's samples from
        return length.value

    def batch_stream_need(self, blocks):
        """[(first, count)] per input: the source frames the next slice of `blocks` blocks must bring."""
        n = self.n_channels
        first, count = (C.c_size_t * n)(), (C.c_size_t * n)()
        self._check(lib().gdg_batch_stream_need(self._h, blocks, first, count))
        return [(first[i], count[i]) for i in range(n)]

    def batch_stream_step(self, blocks, in_bytes, outs=None):
        """One slice: in_bytes[i] = the interleaved frames batch_stream_need asked for (bytes-like or None); returns the N + 3 output
        pieces of blocks * 8192 samples each (uint8 arrays), and one per blend in force behind them.  With a delivery in force a piece has
        batch_delivery_samples(factor, up, down, <session samples of the slices before>, blocks * 8192) samples."""
        n = self.n_channels
        no = n + 3 + self.batch_blends()
        keep = [None if b is None else np.ascontiguousarray(np.frombuffer(b, dtype=np.uint8) if not isinstance(b, np.ndarray) else b, dtype=np.uint8)
                for b in in_bytes]
        assert len(keep) == n
        ins = (C.c_void_p * n)(*[(b.ctypes.data if b is not None and b.size else None) for b in keep])
        size = self._delivered(getattr(self, "_stream_done", 0), blocks * 8192) * self._stream_width
        if outs is None:
            outs = [np.zeros(size, dtype=np.uint8) for _ in range(no)]
        assert len(outs) == no and all(o is None or (o.dtype == np.uint8 and o.size == size) for o in outs)
        ptrs = (C.c_void_p * no)(*[(o.ctypes.data if o is not None else None) for o in outs])
        self._check(lib().gdg_batch_stream_step(self._h, blocks, ins, ptrs))
        self._stream_done = getattr(self, "_stream_done", 0) + blocks * 8192
        return outs

    def batch_stream_close(self):
        self._check(lib().gdg_batch_stream_close(self._h))

    def batch_stream(self, inputs, target_rate, out_format, blocks_per_slice, metronome_to_master=False, run_meters=False, tuner_enqueue=False):
        """batch_run as a generator: the same `inputs` tuples (whole data sections; a real host would read each slice's frames from its
        files instead), cut into slices of `blocks_per_slice` blocks (an int, or a function (blocks_left) -> blocks).  Yields every
        slice's N + 3 output pieces; their concatenation is batch_run's result."""
        metas, datas, widths = self._stream_split(inputs)
        length = self.batch_stream_open(metas, target_rate, out_format, metronome_to_master, run_meters, tuner_enqueue)
        try:
            left = length // 8192
            while left:
                blocks = min(left, blocks_per_slice(left) if callable(blocks_per_slice) else blocks_per_slice)
                need = self.batch_stream_need(blocks)
                ins = [None if d is None or not c else d[f * w:(f + c) * w] for d, w, (f, c) in zip(datas, widths, need)]
                yield self.batch_stream_step(blocks, ins)
                left -= blocks
        finally:
            try:
                self.batch_stream_close()
            except GdgError:
                pass                            # a slice that failed has closed the job itself

    # -- checkpoint / resume of the open streamed job (gdg_batch_stream_checkpoint / _resume, gdg_state_verify) ----------------------
    def batch_stream_checkpoint(self):
        """-> bytes: the open job (plain or a shard's) with everything it carries between slices; the context is not changed."""
        size = C.c_size_t(0)
        self._check(lib().gdg_batch_stream_checkpoint_size(self._h, C.byref(size)))
        buf = C.create_string_buffer(max(size.value, 1))
        written = C.c_size_t(0)
        self._check(lib().gdg_batch_stream_checkpoint(self._h, buf, size.value, C.byref(written)))
        return buf.raw[:written.value]

    def batch_stream_resume(self, inputs, target_rate, out_format, blob, metronome_to_master=False, run_meters=False, tuner_enqueue=False):
        """In the place of batch_stream_open, with its arguments and a checkpoint of that job: returns the samples done.  Nothing changes
        when the blob is rejected."""
        n = len(inputs)
        arr = self._stream_metas(inputs)
        fo = WAVE_FORMATS[out_format] if isinstance(out_format, str) else out_format
        opt = BatchOptions(target_rate, fo, int(bool(metronome_to_master)), int(bool(run_meters)), int(bool(tuner_enqueue)))
        blob = bytes(blob)
        done = C.c_size_t(0)
        self._check(lib().gdg_batch_stream_resume(self._h, arr, n, C.byref(opt), blob, len(blob), C.byref(done)))
        self._stream_width = lib().gdg_wave_bytes_per_sample(fo)
        self._stream_done = done.value
        return done.value

    def batch_stream_resume_shard(self, inputs, target_rate, out_format, blob, job_samples=0, metronome=False, run_meters=False,
                                  tuner_enqueue=False):
        """In the place of batch_stream_open_shard (same job_samples and metronome); returns the samples done."""
        n = len(inputs)
        arr = self._stream_metas(inputs)
        fo = WAVE_FORMATS[out_format] if isinstance(out_format, str) else out_format
        opt = BatchOptions(target_rate, fo, 0, int(bool(run_meters)), int(bool(tuner_enqueue)))
        blob = bytes(blob)
        done = C.c_size_t(0)
        self._check(lib().gdg_batch_stream_resume_shard(self._h, arr, n, C.byref(opt), job_samples, int(bool(metronome)), blob, len(blob),
                                                        C.byref(done)))
        self._stream_width = lib().gdg_wave_bytes_per_sample(fo)
        return done.value

    def state_verify(self, blob):
        """The digest of a checkpoint container, checked on the device; raises GdgError when it does not hold (or for a bare state blob)."""
        blob = bytes(blob)
        self._check(lib().gdg_state_verify(self._h, blob, len(blob)))

    # -- ... and of ONE SHARD of a job split over several contexts (gdg_batch_stream_open_shard / _step_shard, gdg_batch_finish_master_slice)
    def batch_stream_open_shard(self, inputs, target_rate, out_format, job_samples=0, metronome=False, run_meters=False, tuner_enqueue=False,
                                metronome_to_master=False):
        """batch_stream_open for the channels of one shard; `metronome`: this shard runs the job's metronome.  Returns the job's samples
        (metronome_to_master is only there to be refused: the aux input joins the master in batch_finish_master_slice)."""
        n = len(inputs)
        arr = self._stream_metas(inputs)
        fo = WAVE_FORMATS[out_format] if isinstance(out_format, str) else out_format
        opt = BatchOptions(target_rate, fo, int(bool(metronome_to_master)), int(bool(run_meters)), int(bool(tuner_enqueue)))
        length = C.c_size_t(0)
        self._check(lib().gdg_batch_stream_open_shard(self._h, arr, n, C.byref(opt), job_samples, int(bool(metronome)), C.byref(length)))
        self._stream_width = lib().gdg_wave_bytes_per_sample(fo)
        return length.value

    def batch_stream_step_shard(self, blocks, in_bytes, metronome=False, outs=None):
        """One slice of a shard's job: returns (outs, left, right, metronome_bytes, metronome_f64) as batch_run_shard does, of
        blocks * 8192 samples each.  metronome: True, False, or a pair (encoded track?, float64 track?)."""
        n = self.n_channels
        keep = [None if b is None else np.ascontiguousarray(np.frombuffer(b, dtype=np.uint8) if not isinstance(b, np.ndarray) else b, dtype=np.uint8)
                for b in in_bytes]
        assert len(keep) == n
        ins = (C.c_void_p * n)(*[(b.ctypes.data if b is not None and b.size else None) for b in keep])
        count = blocks * 8192
        size = count * self._stream_width
        if outs is None:
            outs = [np.zeros(size, dtype=np.uint8) for _ in range(n)]
        assert len(outs) == n and all(o is None or (o.dtype == np.uint8 and o.size == size) for o in outs)
        ptrs = (C.c_void_p * n)(*[(o.ctypes.data if o is not None else None) for o in outs])
        want_bytes, want_f64 = metronome if isinstance(metronome, tuple) else (metronome, metronome)
        left, right = np.zeros(count), np.zeros(count)
        mb = np.zeros(size, dtype=np.uint8) if want_bytes else None
        mf = np.zeros(count) if want_f64 else None
        so = BatchShardOut(left.ctypes.data, right.ctypes.data, mb.ctypes.data if mb is not None else None,
                           mf.ctypes.data if mf is not None else None, 0)
        self._check(lib().gdg_batch_stream_step_shard(self._h, blocks, ins, ptrs, C.byref(so)))
        return outs, left, right, mb, mf

    def batch_finish_master_slice(self, out_format, lefts, rights, aux=None, sample_rate=0, run_meters=False):
        """batch_finish_master for one slice (whole blocks) of a streamed sharded job: the same code path, hence the same bytes
        (gdg_batch_finish_master_slice)."""
        G, n = len(lefts), lefts[0].size
        fo = WAVE_FORMATS[out_format] if isinstance(out_format, str) else out_format
        wo = lib().gdg_wave_bytes_per_sample(fo)
        lefts = [_f64(a) for a in lefts]
        rights = [_f64(a) for a in rights]
        lp = (C.c_void_p * G)(*[a.ctypes.data for a in lefts])
        rp = (C.c_void_p * G)(*[a.ctypes.data for a in rights])
        ml, mr = np.zeros(n * wo, dtype=np.uint8), np.zeros(n * wo, dtype=np.uint8)
        a = _f64(aux) if aux is not None else None
        self._check(lib().gdg_batch_finish_master_slice(self._h, fo, lp, rp, G, a.ctypes.data if a is not None else None, n, sample_rate,
                                                        int(bool(run_meters)), ml.ctypes.data if n else None, mr.ctypes.data if n else None))
        return ml, mr

    def batch_stream_shard(self, inputs, target_rate, out_format, blocks_per_slice, job_samples=0, metronome=False, run_meters=False,
                           tuner_enqueue=False):
        """batch_run_shard as a generator, in the style of batch_stream: yields (outs, left, right, metronome_bytes, metronome_f64) per
        slice; their concatenation is batch_run_shard's result.  Every shard of a job is sliced alike; the caller finishes each slice's
        master with batch_finish_master_slice."""
        metas, datas, widths = self._stream_split(inputs)
        length = self.batch_stream_open_shard(metas, target_rate, out_format, job_samples, metronome, run_meters, tuner_enqueue)
        try:
            left = length // 8192
            while left:
                blocks = min(left, blocks_per_slice(left) if callable(blocks_per_slice) else blocks_per_slice)
                need = self.batch_stream_need(blocks)
                ins = [None if d is None or not c else d[f * w:(f + c) * w] for d, w, (f, c) in zip(datas, widths, need)]
                yield self.batch_stream_step_shard(blocks, ins, metronome)
                left -= blocks
        finally:
            try:
                self.batch_stream_close()
            except GdgError:
                pass                            # a slice that failed has closed the job itself

    def batch_release(self):
        self._check(lib().gdg_batch_release(self._h))

    # -- the render report: peak, sum of squares and clip counts per output port and block (gdg_block_stats) ---------------------------------
    def block_stats(self, rows, block):
        """rows: a [n_rows][samples] float64 array or a list of equally long 1-D arrays (each row is read where it lies); returns the
        [n_rows][ceil(samples / block)] records (BLOCK_STATS_DTYPE) of gdg_block_stats_rows."""
        if isinstance(rows, np.ndarray) and rows.ndim == 1:
            rows = rows[None, :]
        keep = [_f64(r) for r in rows]
        n = len(keep)
        samples = keep[0].size if n else 0
        assert all(r.ndim == 1 and r.size == samples for r in keep)
        if block < 1:
            raise ValueError("a block has at least one sample")
        out = np.zeros((n, -(-samples // block)), dtype=BLOCK_STATS_DTYPE)
        ptrs = (C.c_void_p * max(n, 1))(*[r.ctypes.data for r in keep])
        self._check(lib().gdg_block_stats_rows(self._h, ptrs, n, samples, block, out.ctypes.data if out.size else None))
        return out

    def block_stats_device(self, d_rows, row_stride, n_rows, samples, block, d_records):
        """gdg_block_stats_rows_device on plain device pointers (ints), enqueued on the context's stream."""
        self._check(lib().gdg_block_stats_rows_device(self._h, d_rows, row_stride, n_rows, samples, block, d_records))

    def batch_report_enable(self, enable=True):
        """From the next batch call on, every batch call keeps the records of what it rendered (configuration: not in a checkpoint)."""
        self._check(lib().gdg_batch_report_enable(self._h, 1 if enable else 0))

    def batch_set_sources(self, source):
        """The source map of the next batch calls (gdg_batch_set_sources): source[c] = the channel whose input entry channel c reads, a list of
        n_channels ints; None (or an empty list) clears it.  A reader's entry in `inputs` may be None; configuration: not in a checkpoint."""
        if source is None or len(source) == 0:
            self._check(lib().gdg_batch_set_sources(self._h, None, 0))
            return
        arr = (C.c_int * len(source))(*[int(v) for v in source])
        self._check(lib().gdg_batch_set_sources(self._h, arr, len(source)))

    def batch_set_dither(self, mode, seed=0, port_base=0):
        """The dither of the LPCM outputs of the next batch calls (gdg_batch_set_dither): mode 0 = off, 1 = TPDF with rounding; the noise of
        a sample depends on (seed, port, sample index) alone; port_base = the job-wide index of this context's first channel.
        Configuration: not in a checkpoint."""
        self._check(lib().gdg_batch_set_dither(self._h, int(mode), int(seed), int(port_base)))

    def batch_dither_seek(self, sample_index):
        """The sample index the next batch_finish_master_slice starts at (gdg_batch_dither_seek)."""
        self._check(lib().gdg_batch_dither_seek(self._h, int(sample_index)))

    def wave_encode_dither(self, fmt, samples, mode=1, seed=0, port=0, first_index=0):
        """A mono row of float64 -> bytes through the dithered encoder (gdg_wave_encode_dither); sample i has index first_index + i."""
        f = WAVE_FORMATS[fmt] if isinstance(fmt, str) else fmt
        x = _f64(samples).reshape(-1)
        out = np.empty(x.size * max(lib().gdg_wave_bytes_per_sample(f), 1), dtype=np.uint8)
        self._check(lib().gdg_wave_encode_dither(self._h, f, x.ctypes.data, x.size, int(mode), int(seed), int(port), int(first_index), out.ctypes.data))
        return out

    def wave_encode_dither_device(self, fmt, d_samples, n, d_bytes, mode=1, seed=0, port=0, first_index=0):
        """gdg_wave_encode_dither_device on plain device pointers (ints), enqueued on the context's stream."""
        f = WAVE_FORMATS[fmt] if isinstance(fmt, str) else fmt
        self._check(lib().gdg_wave_encode_dither_device(self._h, f, d_samples, n, int(mode), int(seed), int(port), int(first_index), d_bytes))

    def batch_set_trim(self, chain_gain=None, master_left=1.0, master_right=1.0, metronome=1.0):
        """The output trim of the next batch calls (gdg_batch_set_trim): a gain per output port in front of the encoders -- chain_gain: one per
        channel of this context (None: all 1), then the job-wide ports.  y = x * g, rounded once, then the encoder; records, meters and
        float64 rows stay as rendered.  All gains 1.0: off.  Configuration: not in a checkpoint."""
        if chain_gain is None:
            self._check(lib().gdg_batch_set_trim(self._h, None, 0, float(master_left), float(master_right), float(metronome)))
            return
        g = np.ascontiguousarray(chain_gain, dtype=np.float64).reshape(-1)
        self._check(lib().gdg_batch_set_trim(self._h, g.ctypes.data if g.size else None, g.size, float(master_left), float(master_right), float(metronome)))

    def wave_encode_trim(self, fmt, samples, gain, mode=0, seed=0, port=0, first_index=0):
        """A mono row of float64 times `gain` -> bytes (gdg_wave_encode_trim): mode 0 the plain encoder, 1 the dithered one; sample i has
        index first_index + i.  gain 1.0 gives wave_encode_dither's bytes."""
        f = WAVE_FORMATS[fmt] if isinstance(fmt, str) else fmt
        x = _f64(samples).reshape(-1)
        out = np.empty(x.size * max(lib().gdg_wave_bytes_per_sample(f), 1), dtype=np.uint8)
        self._check(lib().gdg_wave_encode_trim(self._h, f, x.ctypes.data, x.size, float(gain), int(mode), int(seed), int(port), int(first_index), out.ctypes.data))
        return out

    def wave_encode_trim_device(self, fmt, d_samples, n, d_bytes, gain, mode=0, seed=0, port=0, first_index=0):
        """gdg_wave_encode_trim_device on plain device pointers (ints), enqueued on the context's stream."""
        f = WAVE_FORMATS[fmt] if isinstance(fmt, str) else fmt
        self._check(lib().gdg_wave_encode_trim_device(self._h, f, d_samples, n, float(gain), int(mode), int(seed), int(port), int(first_index), d_bytes))

    @staticmethod
    def _blend_csr(blends):
        """[[(channel, weight), ..], ..] -> (first, channel, weight) as int32 / int32 / float64 arrays; channel and weight carry a spare entry,
        so that lists without a term still have an address and the library can name the empty blend"""
        first = np.zeros(len(blends) + 1, dtype=np.int32)
        first[1:] = np.cumsum([len(b) for b in blends], dtype=np.int64)
        terms = [t for b in blends for t in b]
        return first, np.array([int(t[0]) for t in terms] + [0], dtype=np.int32), np.array([float(t[1]) for t in terms] + [0.0], dtype=np.float64)

    @staticmethod
    def _blend_delays(blends):
        """the delays of terms given as (channel, weight) or (channel, weight, delay): an int32 array with a spare entry, or None where no term has one"""
        terms = [t for b in blends for t in b]
        if not any(len(t) > 2 for t in terms):
            return None
        return np.array([int(t[2]) if len(t) > 2 else 0 for t in terms] + [0], dtype=np.int32)

    @staticmethod
    def _blend_taps(blends):
        """the taps of terms given as (channel, weight, delay, taps): (tap_first int32 [terms + 1], tap float64 with a spare entry), or None
        where no term has a fourth entry"""
        terms = [t for b in blends for t in b]
        if not any(len(t) > 3 for t in terms):
            return None
        taps = [np.asarray(t[3], dtype=np.float64).reshape(-1) if len(t) > 3 and t[3] is not None else np.zeros(0) for t in terms]
        tap_first = np.zeros(len(terms) + 1, dtype=np.int32)
        tap_first[1:] = np.cumsum([h.size for h in taps], dtype=np.int64)
        return tap_first, np.ascontiguousarray(np.concatenate(taps + [np.zeros(1)]), dtype=np.float64)

    def batch_set_blends(self, blends, gain=None):
        """The blend outputs of the next batch calls (gdg_batch_set_blends, gdg_batch_set_blends_delayed, gdg_batch_set_blends_filtered):
        blends = a list of lists of (channel, weight), (channel, weight, delay) or (channel, weight, delay, taps) -- blend b is the sum of its
        terms over this context's chain output rows, in term order, a term with a delay reading its row that many samples back (0 to
        BLEND_MAX_DELAY) and a term with taps (up to BLEND_MAX_TAPS doubles) through that FIR, and port N + 3 + b of every batch call; gain:
        one output gain per blend (None: all 1).  An empty list (or None): off.  Only a list that holds a four-entry term goes through the
        filtered call.  Configuration: not in a checkpoint."""
        blends = [] if blends is None else [list(b) for b in blends]
        if not blends:
            self._check(lib().gdg_batch_set_blends(self._h, 0, None, None, None, None))
            return
        first, channel, weight = self._blend_csr(blends)
        g = None if gain is None else np.ascontiguousarray(gain, dtype=np.float64).reshape(-1)
        if g is not None and g.size != len(blends):
            raise ValueError("%d gains for %d blends" % (g.size, len(blends)))
        delay = self._blend_delays(blends)
        taps = self._blend_taps(blends)
        if taps is not None:
            self._check(lib().gdg_batch_set_blends_filtered(self._h, len(blends), first.ctypes.data, channel.ctypes.data, weight.ctypes.data, delay.ctypes.data,
                                                            taps[0].ctypes.data, taps[1].ctypes.data, None if g is None else g.ctypes.data))
            return
        if delay is not None:
            self._check(lib().gdg_batch_set_blends_delayed(self._h, len(blends), first.ctypes.data, channel.ctypes.data, weight.ctypes.data,
                                                           delay.ctypes.data, None if g is None else g.ctypes.data))
            return
        self._check(lib().gdg_batch_set_blends(self._h, len(blends), first.ctypes.data, channel.ctypes.data,
                                               weight.ctypes.data, None if g is None else g.ctypes.data))

    def batch_blends(self):
        """The number of blends in force (gdg_batch_blends)."""
        return int(lib().gdg_batch_blends(self._h))

    def batch_blend_max_delay(self):
        """The largest delay of the blends in force (gdg_batch_blend_max_delay); 0: the blends are stateless."""
        return int(lib().gdg_batch_blend_max_delay(self._h))

    def batch_blend_max_reach(self):
        """The largest d + max(T, 1) - 1 of the blends in force (gdg_batch_blend_max_reach): how far back a term reads; 0: stateless."""
        return int(lib().gdg_batch_blend_max_reach(self._h))

    def _blend_args(self, blends, parts):
        """the list's pointers in the order of the C calls -- first, channel, weight and then `parts` of "delay", "taps" (two pointers) -- and
        the arrays that keep them alive"""
        first, channel, weight = self._blend_csr(blends)
        delay, taps = self._blend_delays(blends), self._blend_taps(blends)
        args = [first.ctypes.data, channel.ctypes.data, weight.ctypes.data]
        if "delay" in parts:
            args.append(None if delay is None else delay.ctypes.data)
        if "taps" in parts:
            args += [None, None] if taps is None else [taps[0].ctypes.data, taps[1].ctypes.data]
        return args, (first, channel, weight, delay, taps)

    def _blend_rows_host(self, call, parts, rows, blends, history=None):
        """the host form of the three blend calls: rows and the optional history up, [blends, samples] back; the plain call (no parts) takes no history"""
        x = np.ascontiguousarray(rows, dtype=np.float64)
        if x.ndim != 2:
            raise ValueError("rows: [n_rows, samples]")
        blends = [list(b) for b in blends]
        args, keep = self._blend_args(blends, parts)
        h = None if history is None else np.ascontiguousarray(history, dtype=np.float64)
        if h is not None and h.shape != (x.shape[0], BLEND_MAX_DELAY):
            raise ValueError("history: [n_rows, %d]" % BLEND_MAX_DELAY)
        out = np.zeros((len(blends), x.shape[1]), dtype=np.float64)
        rp = (C.c_void_p * max(x.shape[0], 1))(*[x[r].ctypes.data for r in range(x.shape[0])])
        hp = None if h is None else (C.c_void_p * max(x.shape[0], 1))(*[h[r].ctypes.data for r in range(x.shape[0])])
        op = (C.c_void_p * max(len(blends), 1))(*[out[b].ctypes.data for b in range(len(blends))])
        self._check(call(self._h, rp, x.shape[0], x.shape[1], len(blends), *args, *([hp] if parts else []), op))
        return out

    def _blend_rows_device(self, call, parts, d_rows, row_stride, n_rows, samples, blends, d_out, out_stride, history=()):
        """the device form of the three blend calls; history: () or (d_history, hist_stride)"""
        blends = [list(b) for b in blends]
        args, keep = self._blend_args(blends, parts)
        self._check(call(self._h, d_rows, row_stride, n_rows, samples, len(blends), *args, *history, d_out, out_stride))

    def blend_rows_filtered(self, rows, blends, history=None):
        """gdg_blend_rows_filtered: rows [n_rows, samples] float64, blends of (row, weight[, delay[, taps]]) terms, history None (zeros in front
        of sample 0) or [n_rows, BLEND_MAX_DELAY] float64 whose last column is sample -1 -> [blends, samples]."""
        return self._blend_rows_host(lib().gdg_blend_rows_filtered, ("delay", "taps"), rows, blends, history)

    def blend_rows_filtered_device(self, d_rows, row_stride, n_rows, samples, blends, d_out, out_stride, d_history=None, hist_stride=BLEND_MAX_DELAY):
        """gdg_blend_rows_filtered_device on plain device pointers (ints); d_history as blend_rows_delayed_device takes it; returns when the
        sums are written."""
        self._blend_rows_device(lib().gdg_blend_rows_filtered_device, ("delay", "taps"), d_rows, row_stride, n_rows, samples, blends, d_out, out_stride, (d_history, hist_stride))

    def blend_rows_delayed(self, rows, blends, history=None):
        """gdg_blend_rows_delayed: rows [n_rows, samples] float64, blends of (row, weight, delay) terms, history None (zeros in front of sample
        0) or [n_rows, BLEND_MAX_DELAY] float64 whose last column is sample -1 -> [blends, samples]."""
        return self._blend_rows_host(lib().gdg_blend_rows_delayed, ("delay",), rows, blends, history)

    def blend_rows_delayed_device(self, d_rows, row_stride, n_rows, samples, blends, d_out, out_stride, d_history=None, hist_stride=BLEND_MAX_DELAY):
        """gdg_blend_rows_delayed_device on plain device pointers (ints); d_history: None or row r's BLEND_MAX_DELAY samples in front of
        sample 0 at d_history + r * hist_stride; returns when the sums are written."""
        self._blend_rows_device(lib().gdg_blend_rows_delayed_device, ("delay",), d_rows, row_stride, n_rows, samples, blends, d_out, out_stride, (d_history, hist_stride))

    def blend_rows(self, rows, blends):
        """gdg_blend_rows: rows [n_rows, samples] float64, blends as batch_set_blends takes them with `channel` naming a row -> [blends, samples]."""
        return self._blend_rows_host(lib().gdg_blend_rows, (), rows, blends)

    def blend_rows_device(self, d_rows, row_stride, n_rows, samples, blends, d_out, out_stride):
        """gdg_blend_rows_device on plain device pointers (ints); returns when the sums are written."""
        self._blend_rows_device(lib().gdg_blend_rows_device, (), d_rows, row_stride, n_rows, samples, blends, d_out, out_stride)

    # -- the blend fit: Gram records per fit and block, the least-squares weights from them (include/gdg.h, FIT) --------------------------------
    def batch_fit_enable(self, fits):
        """From the next batch call on, every batch call keeps the fit records of what it rendered (gdg_batch_fit_enable): fits = a list of
        (target, [ports]) -- 1 to 8 ports of the call per fit, the chain outputs, master left, master right, metronome and the blend ports
        in force.  None or an empty list: off.  Configuration: not in a checkpoint, refused while a streamed job is open."""
        fits = [] if fits is None else list(fits)
        if not fits:
            self._check(lib().gdg_batch_fit_enable(self._h, 0, None, None, None))
            return
        first, port, target = _fit_csr(fits)
        self._check(lib().gdg_batch_fit_enable(self._h, len(fits), first.ctypes.data, port.ctypes.data, target.ctypes.data))

    def batch_fits(self):
        """The number of fits in force (gdg_batch_fits)."""
        return int(lib().gdg_batch_fits(self._h))

    def batch_fit(self):
        """The [fits][blocks] FIT_DTYPE records of the last completed batch call; GdgError when there are none."""
        fits, blocks = C.c_int(0), C.c_size_t(0)
        self._check(lib().gdg_batch_fit(self._h, None, 0, C.byref(fits), C.byref(blocks)))
        out = np.zeros((fits.value, blocks.value), dtype=FIT_DTYPE)
        self._check(lib().gdg_batch_fit(self._h, out.ctypes.data if out.size else None, out.size, C.byref(fits), C.byref(blocks)))
        return out

    def block_fit(self, rows, fits, block=FIT_BLOCK):
        """gdg_block_fit_rows: rows [n_rows, samples] float64 (or a list of equally long 1-D arrays), fits = (target, [ports]) naming rows ->
        the [fits][ceil(samples / block)] FIT_DTYPE records."""
        if isinstance(rows, np.ndarray) and rows.ndim == 1:
            rows = rows[None, :]
        keep = [_f64(r) for r in rows]
        n = len(keep)
        samples = keep[0].size if n else 0
        assert all(r.ndim == 1 and r.size == samples for r in keep)
        fits = list(fits)
        first, port, target = _fit_csr(fits)
        out = np.zeros((len(fits), -(-samples // int(block)) if int(block) > 0 else 0), dtype=FIT_DTYPE)
        ptrs = (C.c_void_p * max(n, 1))(*[r.ctypes.data for r in keep])
        self._check(lib().gdg_block_fit_rows(self._h, ptrs, n, samples, int(block), len(fits), first.ctypes.data, port.ctypes.data, target.ctypes.data,
                                             out.ctypes.data if out.size else None))
        return out

    def block_fit_device(self, d_rows, row_stride, n_rows, samples, fits, d_records, block=FIT_BLOCK):
        """gdg_block_fit_rows_device on plain device pointers (ints); returns when the records are written."""
        fits = list(fits)
        first, port, target = _fit_csr(fits)
        self._check(lib().gdg_block_fit_rows_device(self._h, d_rows, row_stride, n_rows, samples, int(block), len(fits), first.ctypes.data, port.ctypes.data,
                                                    target.ctypes.data, d_records))

    # -- the Gram of a port list: per block the inner products of all listed rows, on the matrix cores (include/gdg.h, GRAM) ---------------------
    def batch_gram_enable(self, ports):
        """From the next batch call on, every batch call keeps the Gram records of what it rendered (gdg_batch_gram_enable): ports = 2 to 512
        different ports of the call -- chain outputs, master left, master right, metronome, blend ports.  None or an empty list: off.
        Configuration: not in a checkpoint, refused while a streamed job is open."""
        ports = [] if ports is None else [int(p) for p in ports]
        if not ports:
            self._check(lib().gdg_batch_gram_enable(self._h, None, 0))
            return
        port = np.array(ports, dtype=np.int32)
        self._check(lib().gdg_batch_gram_enable(self._h, port.ctypes.data, port.size))

    def batch_gram_ports(self):
        """The Gram list in force (gdg_batch_gram_ports); empty: off."""
        n = int(lib().gdg_batch_gram_ports(self._h, None, 0))
        port = np.zeros(max(n, 1), dtype=np.int32)
        lib().gdg_batch_gram_ports(self._h, port.ctypes.data, n)
        return [int(p) for p in port[:n]]

    def batch_gram(self):
        """The [blocks, P (P + 1) / 2] float64 Gram records of the last completed batch call; GdgError when there are none."""
        blocks = C.c_size_t(0)
        self._check(lib().gdg_batch_gram(self._h, None, 0, C.byref(blocks)))
        n = len(self.batch_gram_ports())
        out = np.zeros((blocks.value, n * (n + 1) // 2), dtype=np.float64)
        self._check(lib().gdg_batch_gram(self._h, out.ctypes.data if out.size else None, out.size, C.byref(blocks)))
        return out

    def block_gram(self, rows, ports, block=GRAM_BLOCK):
        """gdg_block_gram_rows: rows [n_rows, samples] float64 (or a list of equally long 1-D arrays), ports = 1 to 512 different rows ->
        the [ceil(samples / block), P (P + 1) / 2] records."""
        if isinstance(rows, np.ndarray) and rows.ndim == 1:
            rows = rows[None, :]
        keep = [_f64(r) for r in rows]
        n = len(keep)
        samples = keep[0].size if n else 0
        assert all(r.ndim == 1 and r.size == samples for r in keep)
        port = np.array([int(p) for p in ports] + [0], dtype=np.int32)
        P = port.size - 1
        out = np.zeros((-(-samples // int(block)) if int(block) > 0 else 0, P * (P + 1) // 2), dtype=np.float64)
        ptrs = (C.c_void_p * max(n, 1))(*[r.ctypes.data for r in keep])
        self._check(lib().gdg_block_gram_rows(self._h, ptrs, n, samples, int(block), port.ctypes.data, P, out.ctypes.data if out.size else None))
        return out

    def block_gram_device(self, d_rows, row_stride, n_rows, samples, ports, d_records, block=GRAM_BLOCK):
        """gdg_block_gram_rows_device on plain device pointers (ints); returns when the records are written."""
        port = np.array([int(p) for p in ports] + [0], dtype=np.int32)
        self._check(lib().gdg_block_gram_rows_device(self._h, d_rows, row_stride, n_rows, samples, int(block), port.ctypes.data, port.size - 1, d_records))

    # -- the tap fit: per block and fit the Gram of shifted rows, the least-squares taps from it (include/gdg.h, TAPFIT) ------------------------
    def batch_tapfit_enable(self, fits):
        """From the next batch call on, every batch call keeps the tap-fit records of what it rendered (gdg_batch_tapfit_enable): fits = a
        list of (target, [ports], taps) -- 1 to 4 ports of the call per fit, 1 to 64 taps per term, ports x taps <= 128, up to 16 fits.
        None or an empty list: off.  Configuration: not in a checkpoint, refused while a streamed job is open."""
        fits = [] if fits is None else list(fits)
        if not fits:
            self._check(lib().gdg_batch_tapfit_enable(self._h, 0, None, None, None, None))
            return
        first, port, target, taps = _tapfit_csr(fits)
        self._check(lib().gdg_batch_tapfit_enable(self._h, len(fits), first.ctypes.data, port.ctypes.data, target.ctypes.data, taps.ctypes.data))

    def batch_tapfits(self):
        """The number of tap fits in force (gdg_batch_tapfits)."""
        return int(lib().gdg_batch_tapfits(self._h))

    def batch_tapfit(self):
        """The [blocks, D] float64 tap-fit records of the last completed batch call; GdgError when there are none."""
        blocks, per = C.c_size_t(0), C.c_size_t(0)
        self._check(lib().gdg_batch_tapfit(self._h, None, 0, C.byref(blocks), C.byref(per)))
        out = np.zeros((blocks.value, per.value), dtype=np.float64)
        self._check(lib().gdg_batch_tapfit(self._h, out.ctypes.data if out.size else None, out.size, C.byref(blocks), C.byref(per)))
        return out

    def block_tapfit(self, rows, fits, block=TAPFIT_BLOCK):
        """gdg_block_tapfit_rows: rows [n_rows, samples] float64 (or a list of equally long 1-D arrays), fits = (target, [ports], taps) naming
        rows -> the [ceil(samples / block), D] records."""
        if isinstance(rows, np.ndarray) and rows.ndim == 1:
            rows = rows[None, :]
        keep = [_f64(r) for r in rows]
        n = len(keep)
        samples = keep[0].size if n else 0
        assert all(r.ndim == 1 and r.size == samples for r in keep)
        fits = list(fits)
        first, port, target, taps = _tapfit_csr(fits)
        out = np.zeros((-(-samples // int(block)) if int(block) > 0 else 0, tapfit_doubles(fits)), dtype=np.float64)
        ptrs = (C.c_void_p * max(n, 1))(*[r.ctypes.data for r in keep])
        self._check(lib().gdg_block_tapfit_rows(self._h, ptrs, n, samples, int(block), len(fits), first.ctypes.data, port.ctypes.data, target.ctypes.data, taps.ctypes.data,
                                                out.ctypes.data if out.size else None))
        return out

    def block_tapfit_device(self, d_rows, row_stride, n_rows, samples, fits, d_records, block=TAPFIT_BLOCK):
        """gdg_block_tapfit_rows_device on plain device pointers (ints); returns when the records are written."""
        fits = list(fits)
        first, port, target, taps = _tapfit_csr(fits)
        self._check(lib().gdg_block_tapfit_rows_device(self._h, d_rows, row_stride, n_rows, samples, int(block), len(fits), first.ctypes.data, port.ctypes.data,
                                                       target.ctypes.data, taps.ctypes.data, d_records))

    # -- the transfer records: per block and pair the auto- and cross-spectra in groups of bins, match taps from them (include/gdg.h, TRANSFER) --
    def batch_transfer_enable(self, pairs, group=1):
        """From the next batch call on, every batch call keeps the transfer records of what it rendered (gdg_batch_transfer_enable): pairs =
        a list of up to 16 (port, target) of the call, group = the bins summed into one group (1, 2, 4 .. 64).  None or an empty list: off.
        Configuration: not in a checkpoint, refused while a streamed job is open."""
        pairs = [] if pairs is None else list(pairs)
        if not pairs:
            self._check(lib().gdg_batch_transfer_enable(self._h, 0, None, None, int(group)))
            return
        port, target = _transfer_lists(pairs)
        self._check(lib().gdg_batch_transfer_enable(self._h, len(pairs), port.ctypes.data, target.ctypes.data, int(group)))

    def batch_transfers(self):
        """The number of transfer pairs in force (gdg_batch_transfers)."""
        return int(lib().gdg_batch_transfers(self._h))

    def batch_transfer(self):
        """The [blocks, n_pairs x G x 4] float64 transfer records of the last completed batch call; GdgError when there are none."""
        blocks, per = C.c_size_t(0), C.c_size_t(0)
        self._check(lib().gdg_batch_transfer(self._h, None, 0, C.byref(blocks), C.byref(per)))
        out = np.zeros((blocks.value, per.value), dtype=np.float64)
        self._check(lib().gdg_batch_transfer(self._h, out.ctypes.data if out.size else None, out.size, C.byref(blocks), C.byref(per)))
        return out

    def block_transfer(self, rows, pairs, group=1):
        """gdg_block_transfer_rows: rows [n_rows, samples] float64 (or a list of equally long 1-D arrays), pairs = (port, target) naming rows
        -> the [ceil(samples / 8192), n_pairs, 4096 / group + 1, 4] records (Sxx, Syy, Re Sxy, Im Sxy)."""
        if isinstance(rows, np.ndarray) and rows.ndim == 1:
            rows = rows[None, :]
        keep = [_f64(r) for r in rows]
        n = len(keep)
        samples = keep[0].size if n else 0
        assert all(r.ndim == 1 and r.size == samples for r in keep)
        pairs = list(pairs)
        port, target = _transfer_lists(pairs)
        per = transfer_doubles(len(pairs), group)
        out = np.zeros((-(-samples // TRANSFER_BLOCK), per), dtype=np.float64)
        ptrs = (C.c_void_p * max(n, 1))(*[r.ctypes.data for r in keep])
        self._check(lib().gdg_block_transfer_rows(self._h, ptrs, n, samples, len(pairs), port.ctypes.data, target.ctypes.data, int(group), out.ctypes.data if out.size else None))
        return out.reshape(out.shape[0], len(pairs), -1, 4) if per else out

    def block_transfer_device(self, d_rows, row_stride, n_rows, samples, pairs, group, d_records):
        """gdg_block_transfer_rows_device on plain device pointers (ints); returns when the records are written."""
        pairs = list(pairs)
        port, target = _transfer_lists(pairs)
        self._check(lib().gdg_block_transfer_rows_device(self._h, d_rows, row_stride, n_rows, samples, len(pairs), port.ctypes.data, target.ctypes.data, int(group), d_records))

    transfer_doubles = staticmethod(transfer_doubles)

    # -- the delivery: every encoded port of a batch call at a half or a quarter of the session rate (include/gdg.h, DELIVERY) ----------------
    def batch_set_delivery(self, factor):
        """From the next batch call on, batch_run and batch_stream_step write every port at 1 / factor of the session rate
        (gdg_batch_set_delivery): factor 1 (off), 2 or 4.  Each output then has length // factor samples and lags the render by
        batch_delivery_latency(factor) session samples; the records stay those of the session-rate render.  Configuration: not in a
        checkpoint, refused while a streamed job is open; the checkpoint, shard and finish_master calls refuse while it is on."""
        self._check(lib().gdg_batch_set_delivery(self._h, int(factor)))

    def batch_delivery(self):
        """The delivery factor in force (gdg_batch_delivery): 1 = off."""
        return int(lib().gdg_batch_delivery(self._h))

    def deliver_rows(self, rows, factor, history=None):
        """gdg_deliver_rows: rows [n_rows, samples] float64 (or one 1-D row), samples a positive multiple of factor -> [n_rows, samples //
        factor].  history: None (zeros in front of sample 0) or a C-contiguous [n_rows, 154] float64 array, read before and UPDATED IN PLACE
        after, so consecutive calls continue a stream."""
        x = np.ascontiguousarray(rows, dtype=np.float64)
        one = x.ndim == 1
        if one:
            x = x[None, :]
        n, samples = x.shape
        f = int(factor)
        if history is not None:
            assert isinstance(history, np.ndarray) and history.dtype == np.float64 and history.flags.c_contiguous and history.size == n * DELIVER_HISTORY
        out = np.zeros((n, samples // f if f > 0 else 0), dtype=np.float64)
        self._check(lib().gdg_deliver_rows(self._h, x.ctypes.data if x.size else None, n, samples, f, None if history is None else history.ctypes.data,
                                           out.ctypes.data if out.size else None))
        return out[0] if one else out

    def deliver_rows_device(self, d_rows, row_stride, n_rows, samples, factor, d_history, d_out, out_stride):
        """gdg_deliver_rows_device on plain device pointers (ints; d_history 0 or None: zeros in front), enqueued on the context's stream."""
        self._check(lib().gdg_deliver_rows_device(self._h, d_rows, row_stride, n_rows, samples, int(factor), d_history or None, d_out, out_stride))

    def _delivered(self, first, count):
        """the delivered samples of the session samples [first, first + count) under the factor and ratio in force"""
        up, down = self.batch_delivery_ratio()
        return batch_delivery_samples(self.batch_delivery(), up, down, first, count)

    def batch_set_delivery_ratio(self, factor, up, down):
        """From the next batch call on every port leaves at (session rate / factor) * up / down (gdg_batch_set_out_ratio): the factor's
        decimator, then the polyphase ratio stage, in front of the encoders; 44.1 kHz from 192 is (4, 147, 160).  up / down reduced,
        1 <= up <= 160, 1 <= down <= 320, within a factor of two of 1; (factor, 1, 1) is batch_set_delivery(factor).  Each output of a job
        has batch_delivery_samples(factor, up, down, 0, length) samples.  Refused while a streamed job is open; the checkpoint, shard and
        finish_master calls refuse while a ratio is in force."""
        self._check(lib().gdg_batch_set_out_ratio(self._h, int(factor), int(up), int(down)))

    def batch_delivery_ratio(self):
        """(up, down) of the delivery ratio in force (gdg_batch_out_ratio): (1, 1) = none."""
        up, down = C.c_int(1), C.c_int(1)
        lib().gdg_batch_out_ratio(self._h, C.byref(up), C.byref(down))
        return up.value, down.value

    def deliver_rows_ratio(self, rows, up, down, first=0, history=None):
        """gdg_out_ratio_rows: rows [n_rows, samples] float64 (or one 1-D row), the intermediate samples [first, first + samples) of a
        job -> [n_rows, ceil((first + samples) up / down) - ceil(first up / down)].  history: None (zeros in front of the call) or a
        C-contiguous [n_rows, 127] float64 array, read before and UPDATED IN PLACE after, so consecutive calls with advancing first continue
        a stream."""
        x = np.ascontiguousarray(rows, dtype=np.float64)
        one = x.ndim == 1
        if one:
            x = x[None, :]
        n, samples = x.shape
        up, down, first = int(up), int(down), int(first)
        if history is not None:
            assert isinstance(history, np.ndarray) and history.dtype == np.float64 and history.flags.c_contiguous and history.size == n * DELIVER_RATIO_HISTORY
        n_out = samples if (up, down) == (1, 1) else batch_delivery_samples(1, up, down, first, samples)
        out = np.zeros((n, n_out), dtype=np.float64)
        self._check(lib().gdg_out_ratio_rows(self._h, x.ctypes.data if x.size else None, n, samples, up, down, first, None if history is None else history.ctypes.data,
                                                 out.ctypes.data if out.size else None, n_out))
        return out[0] if one else out

    def deliver_rows_ratio_device(self, d_rows, row_stride, n_rows, samples, up, down, first, d_history, d_out, out_stride):
        """gdg_out_ratio_rows_device on plain device pointers (ints; d_history 0 or None: zeros in front), enqueued on the context's stream."""
        self._check(lib().gdg_out_ratio_rows_device(self._h, d_rows, row_stride, n_rows, samples, int(up), int(down), int(first), d_history or None, d_out, out_stride))

    batch_delivery_samples = staticmethod(batch_delivery_samples)
    batch_delivery_ratio_latency = staticmethod(batch_delivery_ratio_latency)
    deliver_ratio_taps = staticmethod(deliver_ratio_taps)
    batch_delivery_latency = staticmethod(batch_delivery_latency)
    deliver_taps = staticmethod(deliver_taps)
    match_taps_from_transfer = staticmethod(match_taps_from_transfer)

    def batch_report(self):
        """The [ports][blocks] records (BLOCK_STATS_DTYPE) of the last completed batch call; GdgError when there is none."""
        ports, blocks = C.c_int(0), C.c_size_t(0)
        self._check(lib().gdg_batch_report(self._h, None, 0, C.byref(ports), C.byref(blocks)))
        out = np.zeros((ports.value, blocks.value), dtype=BLOCK_STATS_DTYPE)
        self._check(lib().gdg_batch_report(self._h, out.ctypes.data if out.size else None, out.size, C.byref(ports), C.byref(blocks)))
        return out

    # -- the band spectrum: the power per output port, block of 8192 samples and frequency band (include/gdg.h) ------------------------------
    def block_spectrum(self, rows, sample_rate, edges):
        """rows: a [n_rows][samples] float64 array or a list of equally long 1-D arrays; returns the [n_rows][ceil(samples / 8192)][bands]
        float64 array of gdg_block_spectrum_rows for the len(edges) - 1 bands between the edges (Hz)."""
        e = spectrum_edges(edges)
        if int(sample_rate) <= 0:
            raise ValueError("sample rate must be positive")
        if isinstance(rows, np.ndarray) and rows.ndim == 1:
            rows = rows[None, :]
        keep = [_f64(r) for r in rows]
        n = len(keep)
        samples = keep[0].size if n else 0
        assert all(r.ndim == 1 and r.size == samples for r in keep)
        out = np.zeros((n, -(-samples // SPECTRUM_BLOCK), e.size - 1), dtype=np.float64)
        ptrs = (C.c_void_p * max(n, 1))(*[r.ctypes.data for r in keep])
        self._check(lib().gdg_block_spectrum_rows(self._h, ptrs, n, samples, int(sample_rate), e.ctypes.data, e.size, out.ctypes.data if out.size else None))
        return out

    def block_spectrum_device(self, d_rows, row_stride, n_rows, samples, sample_rate, edges, d_bands):
        """gdg_block_spectrum_rows_device on plain device pointers (ints), enqueued on the context's stream; the edges are host values."""
        e = spectrum_edges(edges)
        self._check(lib().gdg_block_spectrum_rows_device(self._h, d_rows, row_stride, n_rows, samples, int(sample_rate), e.ctypes.data, e.size, d_bands))

    def batch_spectrum_enable(self, edges):
        """From the next batch call on, every batch call keeps the band powers of what it rendered, for the bands between `edges` (Hz) at the
        job's rate; None (or an empty list) switches it off.  Configuration: not in a checkpoint, refused while a streamed job is open."""
        if edges is None or len(edges) == 0:
            self._check(lib().gdg_batch_spectrum_enable(self._h, None, 0))
            return
        e = spectrum_edges(edges)
        self._check(lib().gdg_batch_spectrum_enable(self._h, e.ctypes.data, e.size))

    def batch_spectrum(self):
        """The [ports][blocks][bands] float64 band powers of the last completed batch call; GdgError when there is none."""
        ports, blocks, bands = C.c_int(0), C.c_size_t(0), C.c_int(0)
        self._check(lib().gdg_batch_spectrum(self._h, None, 0, C.byref(ports), C.byref(blocks), C.byref(bands)))
        out = np.zeros((ports.value, blocks.value, bands.value), dtype=np.float64)
        self._check(lib().gdg_batch_spectrum(self._h, out.ctypes.data if out.size else None, out.size, C.byref(ports), C.byref(blocks), C.byref(bands)))
        return out

    # -- the alignment report: lag and polarity per output port and block of 8192 samples against a reference port (include/gdg.h) ------------
    def block_align(self, rows, ref, max_lag):
        """rows: a [n_rows][samples] float64 array or a list of equally long 1-D arrays; ref[r]: -1 or the row that row r is measured
        against; returns the [n_rows][ceil(samples / 8192)] BLOCK_ALIGN_DTYPE records of gdg_block_align_rows."""
        if isinstance(rows, np.ndarray) and rows.ndim == 1:
            rows = rows[None, :]
        keep = [_f64(r) for r in rows]
        n = len(keep)
        refs = align_refs(ref, max_lag)
        if refs.size != n:
            raise ValueError("%d references for %d rows" % (refs.size, n))
        samples = keep[0].size
        assert all(r.ndim == 1 and r.size == samples for r in keep)
        out = np.zeros((n, -(-samples // ALIGN_BLOCK)), dtype=BLOCK_ALIGN_DTYPE)
        ptrs = (C.c_void_p * n)(*[r.ctypes.data for r in keep])
        self._check(lib().gdg_block_align_rows(self._h, ptrs, n, samples, refs.ctypes.data, int(max_lag), out.ctypes.data if out.size else None))
        return out

    def block_align_device(self, d_rows, row_stride, n_rows, samples, ref, max_lag, d_records):
        """gdg_block_align_rows_device on plain device pointers (ints), enqueued on the context's stream; the references are host values."""
        refs = align_refs(ref, max_lag)
        if refs.size != n_rows:
            raise ValueError("%d references for %d rows" % (refs.size, n_rows))
        self._check(lib().gdg_block_align_rows_device(self._h, d_rows, row_stride, n_rows, samples, refs.ctypes.data, int(max_lag), d_records))

    def batch_align_enable(self, ref, max_lag=ALIGN_MAX_LAG):
        """From the next batch call on, every batch call keeps the alignment records of what it rendered: port p against port ref[p] (-1:
        not measured), one entry per port of the calls to come; None (or an empty list) switches it off.  Configuration: not in a
        checkpoint, refused while a streamed job is open."""
        if ref is None or len(ref) == 0:
            self._check(lib().gdg_batch_align_enable(self._h, None, 0, 0))
            return
        refs = align_refs(ref, max_lag)
        self._check(lib().gdg_batch_align_enable(self._h, refs.ctypes.data, refs.size, int(max_lag)))

    def batch_align(self):
        """The [ports][blocks] BLOCK_ALIGN_DTYPE records of the last completed batch call; GdgError when there are none."""
        ports, blocks = C.c_int(0), C.c_size_t(0)
        self._check(lib().gdg_batch_align(self._h, None, 0, C.byref(ports), C.byref(blocks)))
        out = np.zeros((ports.value, blocks.value), dtype=BLOCK_ALIGN_DTYPE)
        self._check(lib().gdg_batch_align(self._h, out.ctypes.data if out.size else None, out.size, C.byref(ports), C.byref(blocks)))
        return out

    # -- the true-peak record: the 4x oversampled peak per output port and block of 8192 samples (include/gdg.h) -----------------------------
    def block_true_peak(self, rows):
        """rows: a [n_rows][samples] float64 array or a list of equally long 1-D arrays; returns the [n_rows][ceil(samples / 8192)]
        BLOCK_TRUE_PEAK_DTYPE records of gdg_block_true_peak_rows."""
        if isinstance(rows, np.ndarray) and rows.ndim == 1:
            rows = rows[None, :]
        keep = [_f64(r) for r in rows]
        n = len(keep)
        samples = keep[0].size if n else 0
        assert all(r.ndim == 1 and r.size == samples for r in keep)
        out = np.zeros((n, -(-samples // TRUE_PEAK_BLOCK)), dtype=BLOCK_TRUE_PEAK_DTYPE)
        ptrs = (C.c_void_p * max(n, 1))(*[r.ctypes.data for r in keep])
        self._check(lib().gdg_block_true_peak_rows(self._h, ptrs, n, samples, out.ctypes.data if out.size else None))
        return out

    def block_true_peak_device(self, d_rows, row_stride, n_rows, samples, d_records):
        """gdg_block_true_peak_rows_device on plain device pointers (ints), enqueued on the context's stream."""
        self._check(lib().gdg_block_true_peak_rows_device(self._h, d_rows, row_stride, n_rows, samples, d_records))

    def batch_true_peak_enable(self, enable=True):
        """From the next batch call on, every batch call keeps the true-peak records of what it rendered (off by default).  Configuration:
        not in a checkpoint, refused while a streamed job is open."""
        self._check(lib().gdg_batch_true_peak_enable(self._h, 1 if enable else 0))

    def batch_true_peak(self):
        """The [ports][blocks] BLOCK_TRUE_PEAK_DTYPE records of the last completed batch call; GdgError when there are none."""
        ports, blocks = C.c_int(0), C.c_size_t(0)
        self._check(lib().gdg_batch_true_peak(self._h, None, 0, C.byref(ports), C.byref(blocks)))
        out = np.zeros((ports.value, blocks.value), dtype=BLOCK_TRUE_PEAK_DTYPE)
        self._check(lib().gdg_batch_true_peak(self._h, out.ctypes.data if out.size else None, out.size, C.byref(ports), C.byref(blocks)))
        return out

    # -- the records of the delivered rows: peak, sum of squares and a true peak that is seamless across blocks of any length (include/gdg.h) --
    def block_delivered_rows(self, rows, span, history=None):
        """gdg_block_out_rows: rows [n_rows][samples] float64 (or a list of equally long 1-D arrays, or one 1-D row) cut into blocks by
        span[0 .. n_blocks] (ascending, span[0] = 0, span[-1] = samples, lengths 1 to 16384); returns the [n_rows][n_blocks]
        BLOCK_DELIVERED_DTYPE records.  history: None (zeros stand in front, nothing is kept) or a C-contiguous [n_rows, 23] float64 array,
        read before and UPDATED IN PLACE after, so consecutive calls continue a stream."""
        if isinstance(rows, np.ndarray) and rows.ndim == 1:
            rows = rows[None, :]
        keep = [_f64(r) for r in rows]
        n = len(keep)
        samples = keep[0].size if n else 0
        assert all(r.ndim == 1 and r.size == samples for r in keep)
        sp = np.ascontiguousarray(span, dtype=np.uint64)
        assert sp.ndim == 1 and sp.size >= 1
        if history is not None:
            assert isinstance(history, np.ndarray) and history.dtype == np.float64 and history.flags.c_contiguous and history.size == n * DELIVERED_HISTORY
        out = np.zeros((n, sp.size - 1), dtype=BLOCK_DELIVERED_DTYPE)
        ptrs = (C.c_void_p * max(n, 1))(*[r.ctypes.data for r in keep])
        self._check(lib().gdg_block_out_rows(self._h, ptrs, n, samples, sp.ctypes.data, sp.size - 1, None if history is None else history.ctypes.data,
                                             out.ctypes.data if out.size else None))
        return out

    def block_delivered_rows_device(self, d_rows, row_stride, n_rows, samples, span, d_history, d_records):
        """gdg_block_out_rows_device on plain device pointers (ints; d_history 0 or None: zeros in front); span is a host sequence.  Enqueued
        on the context's stream."""
        sp = np.ascontiguousarray(span, dtype=np.uint64)
        self._check(lib().gdg_block_out_rows_device(self._h, d_rows, row_stride, n_rows, samples, sp.ctypes.data, sp.size - 1, d_history or None, d_records))

    def batch_delivered_enable(self, enable=True):
        """From the next batch call on, batch_run and batch_stream_step keep the records of the rows the encoders read -- the delivered rows,
        in front of any gain -- of every encoded port (gdg_batch_out_records_enable; off by default).  Configuration: not in a checkpoint,
        refused while a streamed job is open; the checkpoint, shard and finish_master calls refuse while it is on."""
        self._check(lib().gdg_batch_out_records_enable(self._h, 1 if enable else 0))

    def batch_delivered(self):
        """The [ports][blocks] BLOCK_DELIVERED_DTYPE records of the last completed batch call; GdgError when there are none."""
        ports, blocks = C.c_int(0), C.c_size_t(0)
        self._check(lib().gdg_batch_out_records(self._h, None, 0, C.byref(ports), C.byref(blocks)))
        out = np.zeros((ports.value, blocks.value), dtype=BLOCK_DELIVERED_DTYPE)
        self._check(lib().gdg_batch_out_records(self._h, out.ctypes.data if out.size else None, out.size, C.byref(ports), C.byref(blocks)))
        return out

    trim_from_delivered = staticmethod(trim_from_delivered)

    def loudness_rows(self, rows, rate, first=0, state=None):
        """gdg_loudness_rows: rows [n_rows][count] float64 (or one 1-D row), the samples [first, first + count) of a stream at `rate`.  Returns
        (records [n_rows][hops] -- the hop sums of the K-weighted samples that complete in them --, state [n_rows][LOUDNESS_STATE_DOUBLES]).
        state None starts a stream (first must be 0); a continuing call passes the state the call before returned and begins at a multiple of
        LOUDNESS_TILE samples."""
        x = np.ascontiguousarray(rows, dtype=np.float64)
        if x.ndim == 1:
            x = x[None, :]
        if x.ndim != 2:
            raise ValueError("rows: [n_rows, count]")
        n, count = x.shape
        st_in = None if state is None else np.ascontiguousarray(state, dtype=np.float64)
        if st_in is not None and st_in.shape != (n, LOUDNESS_STATE_DOUBLES):
            raise ValueError("state: [n_rows, %d]" % LOUDNESS_STATE_DOUBLES)
        hops = loudness_hops(rate, first, count)
        out, st_out = np.zeros((n, hops), dtype=np.float64), np.zeros((n, LOUDNESS_STATE_DOUBLES), dtype=np.float64)
        self._check(lib().gdg_loudness_rows(self._h, x.ctypes.data if x.size else None, count, n, int(first), count, int(rate), None if st_in is None else st_in.ctypes.data,
                                            st_out.ctypes.data, out.ctypes.data if out.size else None, hops))
        return out, st_out

    def loudness_rows_device(self, d_rows, row_stride, n_rows, first, count, rate, d_state_in, d_state_out, d_records, records_stride):
        """gdg_loudness_rows_device on plain device pointers (ints; d_state_in 0 or None starts a stream).  Enqueued on the context's stream."""
        self._check(lib().gdg_loudness_rows_device(self._h, d_rows, row_stride, n_rows, first, count, int(rate), d_state_in or None, d_state_out or None, d_records or None,
                                                   records_stride))

    def batch_loudness_enable(self, enable=True):
        """From the next batch call on, batch_run and batch_stream_step keep the hop records -- the sum of squares of the K-weighted samples of
        every 100 ms -- of every encoded port, taken from the session-rate rows in front of delivery, trim and blend gain
        (gdg_batch_loudness_enable; off by default).  Configuration: not in a checkpoint, refused while a streamed job is open; the checkpoint,
        shard and finish_master calls refuse while it is on."""
        self._check(lib().gdg_batch_loudness_enable(self._h, 1 if enable else 0))

    def batch_loudness(self):
        """The [ports][hops] float64 hop records of the last completed batch call or slice; GdgError when there are none."""
        ports, hops = C.c_int(0), C.c_size_t(0)
        self._check(lib().gdg_batch_loudness(self._h, None, 0, C.byref(ports), C.byref(hops)))
        out = np.zeros((ports.value, hops.value), dtype=np.float64)
        self._check(lib().gdg_batch_loudness(self._h, out.ctypes.data if out.size else None, out.size, C.byref(ports), C.byref(hops)))
        return out

    loudness_from_hops = staticmethod(loudness_from_hops)
    trim_from_loudness = staticmethod(trim_from_loudness)
    loudness_hops = staticmethod(loudness_hops)
    loudness_coefficients = staticmethod(loudness_coefficients)

    def metronome_process(self, frames):
        out = np.empty(frames, dtype=np.float64)
        self._check(lib().gdg_metronome_process(self._h, out.ctypes.data, frames))
        return out
