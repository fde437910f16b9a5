"""ctypes binding of libgdg_host.so: the C++ mirror of effects.Unit / signal.Chain (host/gdg_host.hpp).

Test and bench plumbing only; the mirrored interface itself is the C++ one (and its Go twin in go/).
A Go `error` comes back as a Python exception (HostError) carrying the reference's message text.
"""
import collections
import ctypes as C
import math
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libgdg_host.so")


class HostError(RuntimeError):
    pass


def build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(_HERE, "host")])
    return LIB_PATH


_lib = None
ATTENUATION_HALF_DECIBEL = 0.9440608762859234      # what the delivery factor's decimator multiplies by (csrc/deliver.h, GDG_DELIVER_ATTENUATION)

# The nine kinds of records a batch call keeps, in the order the batch calls fetch them.  attr: the Engine attribute that holds the last
# call's; getter: the gdgh_ function; dtype: the name of a package constant, or "float64"; counts: what the getter reports behind (records,
# capacity); shape: the array's shape over those counts; axis: the one along which a streamed job's slices are joined
RecordKind = collections.namedtuple("RecordKind", "attr getter dtype counts shape axis")
_PORTS_BLOCKS = ((C.c_int, C.c_size_t), lambda rows, blocks: (rows, blocks), 1)
_BLOCKS_PER = ((C.c_size_t, C.c_size_t), lambda blocks, per: (blocks, per), 0)
RECORD_KINDS = {
    "report": RecordKind("last_report", "gdgh_engine_last_batch_report", "BLOCK_STATS_DTYPE", *_PORTS_BLOCKS),
    "spectrum": RecordKind("last_spectrum", "gdgh_engine_last_batch_spectrum", "float64", (C.c_int, C.c_size_t, C.c_int), lambda ports, blocks, bands: (ports, blocks, bands), 1),
    "align": RecordKind("last_align", "gdgh_engine_last_batch_align", "BLOCK_ALIGN_DTYPE", *_PORTS_BLOCKS),
    "true_peak": RecordKind("last_true_peak", "gdgh_engine_last_batch_true_peak", "BLOCK_TRUE_PEAK_DTYPE", *_PORTS_BLOCKS),
    "fit": RecordKind("last_fit", "gdgh_engine_last_batch_fit", "FIT_DTYPE", *_PORTS_BLOCKS),
    "gram": RecordKind("last_gram", "gdgh_engine_last_batch_gram", "float64", (C.c_int, C.c_size_t), lambda ports, blocks: (blocks, ports * (ports + 1) // 2), 0),
    "tapfit": RecordKind("last_tapfit", "gdgh_engine_last_batch_tapfit", "float64", *_BLOCKS_PER),
    "transfer": RecordKind("last_transfer", "gdgh_engine_last_batch_transfer", "float64", *_BLOCKS_PER),
    "delivered": RecordKind("last_delivered", "gdgh_engine_last_batch_delivered", "BLOCK_DELIVERED_DTYPE", *_PORTS_BLOCKS),
}


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HostError("libgdg_host.so is not built")
        # libgdg.so first so that the host library's NEEDED entry resolves to the in-tree copy
        C.CDLL(os.path.join(_HERE, "lib", "libgdg.so"), mode=C.RTLD_GLOBAL)
        L = C.CDLL(LIB_PATH)
        vp, i32, cs = C.c_void_p, C.c_int, C.c_char_p
        sig = {
            "gdgh_engine_create": (vp, [i32, i32, i32]), "gdgh_engine_destroy": (None, [vp]),
            "gdgh_engine_set_rendezvous": (None, [vp, i32, i32]), "gdgh_engine_last_error": (cs, [vp]),
            "gdgh_engine_process_all": (cs, [vp, vp, vp, i32, C.c_uint32]),
            "gdgh_engine_batch_run": (cs, [vp, vp, i32, vp, i32, vp, C.POINTER(C.c_size_t)]),
            "gdgh_engine_batch_stream_open": (cs, [vp, vp, i32, vp, i32, C.POINTER(C.c_size_t)]),
            "gdgh_engine_batch_stream_need": (cs, [vp, i32, vp, vp]), "gdgh_engine_batch_stream_step": (cs, [vp, i32, vp, vp]),
            "gdgh_engine_batch_stream_close": (cs, [vp]),
            "gdgh_engine_batch_stream_sharded_open": (cs, [vp, vp, i32, vp, i32, C.POINTER(C.c_size_t)]),
            "gdgh_engine_batch_stream_sharded_need": (cs, [vp, i32, vp, vp]), "gdgh_engine_batch_stream_sharded_step": (cs, [vp, i32, vp, vp]),
            "gdgh_engine_batch_stream_sharded_close": (cs, [vp]),
            "gdgh_engine_set_batch_report": (None, [vp, i32]),
            "gdgh_engine_set_batch_dither": (None, [vp, i32, C.c_uint64]),
            "gdgh_engine_set_batch_trim": (cs, [vp, vp, i32, C.c_double, C.c_double, C.c_double]),
            "gdgh_engine_set_batch_delivery": (cs, [vp, i32]),
            "gdgh_engine_batch_delivery": (i32, [vp]),
            "gdgh_engine_set_batch_delivery_ratio": (cs, [vp, i32, i32, i32]),
            "gdgh_engine_batch_delivery_ratio": (None, [vp, vp, vp]),
            "gdgh_engine_sync_chains": (cs, [vp, C.c_uint32]),
            "gdgh_engine_set_batch_blends": (cs, [vp, i32, vp, vp, vp, vp]),
            "gdgh_engine_batch_blends": (i32, [vp]),
            "gdgh_engine_set_batch_fits": (cs, [vp, i32, vp, vp, vp]),
            "gdgh_engine_batch_fits": (i32, [vp]),
            "gdgh_engine_set_batch_gram": (cs, [vp, vp, i32]),
            "gdgh_engine_batch_gram_ports": (i32, [vp]),
            "gdgh_engine_set_batch_tapfits": (cs, [vp, i32, vp, vp, vp, vp]),
            "gdgh_engine_batch_tapfits": (i32, [vp]),
            "gdgh_engine_set_batch_transfers": (cs, [vp, i32, vp, vp, i32]),
            "gdgh_engine_batch_transfers": (i32, [vp]),
            "gdgh_engine_set_batch_delivered": (cs, [vp, i32]),
            "gdgh_engine_set_batch_loudness": (cs, [vp, i32]),
            "gdgh_engine_last_batch_loudness": (cs, [vp, vp, C.c_size_t, C.POINTER(i32), C.POINTER(C.c_size_t)]),
            "gdgh_engine_set_batch_blends_delayed": (cs, [vp, i32, vp, vp, vp, vp, vp]),
            "gdgh_engine_set_batch_blends_filtered": (cs, [vp, i32, vp, vp, vp, vp, vp, vp, vp]),
            "gdgh_engine_batch_stream_sharded_checkpoint": (cs, [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]),
            "gdgh_engine_batch_stream_sharded_resume": (cs, [vp, vp, i32, vp, i32, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
            "gdgh_engine_set_batch_sources": (cs, [vp, vp, i32]),
            "gdgh_engine_set_batch_spectrum": (cs, [vp, vp, i32]),
            "gdgh_engine_set_batch_align": (cs, [vp, vp, i32, i32]),
            "gdgh_engine_set_batch_true_peak": (None, [vp, i32]),
            "gdgh_engine_context": (vp, [vp, i32]), "gdgh_engine_shard_range": (None, [vp, i32, C.POINTER(i32), C.POINTER(i32)]),
            "gdgh_engine_create_sharded": (vp, [i32, i32, vp, i32]), "gdgh_engine_shards": (i32, [vp]), "gdgh_engine_shard_of": (i32, [vp, i32]),
            "gdgh_engine_save_state": (cs, [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]),
            "gdgh_engine_load_state": (cs, [vp, vp, C.c_size_t, C.c_uint32]), "gdgh_free": (None, [vp]),
            "gdgh_spatializer_create": (vp, [vp, C.c_uint32]), "gdgh_spatializer_destroy": (None, [vp]),
            "gdgh_spatializer_set": (cs, [vp, i32, C.c_uint32, C.c_double]), "gdgh_spatializer_get": (cs, [vp, i32, C.c_uint32, C.POINTER(C.c_double)]),
            "gdgh_spatializer_input_count": (C.c_uint32, [vp]), "gdgh_spatializer_output_count": (C.c_uint32, [vp]),
            "gdgh_spatializer_set_sample_rate": (None, [vp, C.c_uint32]),
            "gdgh_spatializer_process": (None, [vp, vp, vp, vp, vp, i32, i32]),
            "gdgh_tuner_create": (vp, [i32]), "gdgh_tuner_destroy": (None, [vp]), "gdgh_tuner_process": (None, [vp, vp, i32, C.c_uint32]),
            "gdgh_tuner_analyze": (cs, [vp, C.POINTER(i32), C.POINTER(C.c_double), vp, i32]),
            "gdgh_irs_create": (vp, []), "gdgh_irs_destroy": (None, [vp]),
            "gdgh_irs_add": (None, [vp, cs, C.c_uint32, C.c_int32, vp, i32]),
            "gdgh_chain_create": (vp, [vp, vp]), "gdgh_chain_destroy": (None, [vp]),
            "gdgh_chain_append_unit": (cs, [vp, i32, C.POINTER(i32)]), "gdgh_chain_remove_unit": (cs, [vp, i32]),
            "gdgh_chain_move_up": (cs, [vp, i32]), "gdgh_chain_move_down": (cs, [vp, i32]),
            "gdgh_chain_unit_type": (cs, [vp, i32, C.POINTER(i32)]), "gdgh_chain_set_bypass": (cs, [vp, i32, i32]),
            "gdgh_chain_get_bypass": (cs, [vp, i32, C.POINTER(i32)]),
            "gdgh_chain_set_discrete": (cs, [vp, i32, cs, cs]), "gdgh_chain_get_discrete": (cs, [vp, i32, cs, vp, i32]),
            "gdgh_chain_set_numeric": (cs, [vp, i32, cs, C.c_int32]), "gdgh_chain_get_numeric": (cs, [vp, i32, cs, C.POINTER(C.c_int32)]),
            "gdgh_chain_length": (i32, [vp]), "gdgh_chain_parameters": (cs, [vp, i32, vp, i32]),
            "gdgh_chain_process": (None, [vp, vp, i32, vp, i32, C.c_uint32]),
            "gdgh_unit_create": (vp, [i32]), "gdgh_unit_destroy": (None, [vp]),
            "gdgh_unit_set_numeric": (cs, [vp, cs, C.c_int32]), "gdgh_unit_set_discrete": (cs, [vp, cs, cs]),
            "gdgh_unit_process": (None, [vp, vp, vp, i32, C.c_uint32]),
            "gdgh_filter_compile": (i32, [vp, i32, C.c_uint32, C.c_int32, C.c_uint32, C.c_int32, vp, i32]),
        }
        for row in RECORD_KINDS.values():
            sig[row.getter] = (cs, [vp, vp, C.c_size_t] + [C.POINTER(t) for t in row.counts])
        for name, (res, args) in sig.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _err(msg):
    if msg is not None:
        raise HostError(msg.decode())


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class ImpulseResponses:
    """filter.ImpulseResponses filled from memory (the reference imports WAV files, out of scope)."""

    def __init__(self):
        self._h = lib().gdgh_irs_create()

    def add(self, name, sample_rate, compensation_db, taps):
        t = _f64(taps)
        lib().gdgh_irs_add(self._h, name.encode(), sample_rate, compensation_db, t.ctypes.data, t.size)


class Engine:
    def __init__(self, n_channels, max_frames=8192, device=0, devices=None):
        """devices: one shard (context) per entry -- the same device may appear several times (independent contexts)."""
        if devices is None:
            self._h = lib().gdgh_engine_create(n_channels, max_frames, device)
        else:
            arr = (C.c_int * len(devices))(*devices)
            self._h = lib().gdgh_engine_create_sharded(n_channels, max_frames, arr, len(devices))
        self.n_channels = n_channels
        self.chains = []
        self.last_report = None          # the render report of the last batch call made with report=True: [N + 3, blocks] records
        self.last_spectrum = None        # the band spectrum of the last batch call made with spectrum=edges: [N + 3, blocks, bands] float64
        self.last_true_peak = None       # the true-peak records of the last batch call made with true_peak=True: [N + 3, blocks] records
        self.last_fit = None             # the fit records of the last batch call made with fits=: [fits, blocks] records (FIT_DTYPE)
        self.last_gram = None            # the Gram records of the last batch call made with gram=: [blocks, P (P + 1) / 2] float64
        self.last_transfer = None        # the transfer records of the last batch call made with transfers=: [blocks, pairs x G x 4] float64
        self.last_tapfit = None          # the tap-fit records of the last batch call made with tapfits=: [blocks, D] float64
        self.last_delivered = None       # the records of the delivered rows of the last batch call made with delivered=True: [N + 3 + B, blocks] records
        self.normalize_delivered = None  # ... and those of render_normalized(measure="delivered")'s measuring pass
        self.last_loudness = None        # the loudness records of the last batch call made with loudness=True: [N + 3 + B, hops] float64 hop sums
        self.normalize_loudness = None   # ... those of render_normalized(measure="loudness")'s measuring pass,
        self.normalize_capped = None     # ... and which of its ports' gains the true-peak ceiling capped
        self.last_align = None           # the alignment records of the last batch call made with align=(ref, max_lag): [N + 3, blocks] records

    def shards(self):
        return lib().gdgh_engine_shards(self._h)

    def shard_of(self, channel):
        return lib().gdgh_engine_shard_of(self._h, channel)

    def close(self):
        if getattr(self, "_h", None):
            for c in self.chains:
                c._close()
            lib().gdgh_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def set_rendezvous(self, expected, timeout_ms):
        lib().gdgh_engine_set_rendezvous(self._h, expected, timeout_ms)

    def last_error(self):
        return lib().gdgh_engine_last_error(self._h).decode()

    def create_chain(self, irs=None):
        h = lib().gdgh_chain_create(self._h, irs._h if irs is not None else None)
        if not h:
            raise HostError("CreateChain failed")
        c = Chain(h, irs)
        self.chains.append(c)
        return c

    def process_all(self, x, sample_rate):
        x = _f64(x)
        n = x.shape[0]
        out = np.empty_like(x)
        ins = (C.c_void_p * n)(*[x[i].ctypes.data for i in range(n)])
        outs = (C.c_void_p * n)(*[out[i].ctypes.data for i in range(n)])
        _err(lib().gdgh_engine_process_all(self._h, ins, outs, x.shape[1], sample_rate))
        return out


    def save_state(self):
        """Engine::SaveState -> bytes (every channel of the engine)"""
        p, n = C.c_void_p(), C.c_size_t(0)
        _err(lib().gdgh_engine_save_state(self._h, C.byref(p), C.byref(n)))
        try:
            return C.string_at(p, n.value)
        finally:
            lib().gdgh_free(p)

    def load_state(self, blob, sample_rate):
        """Engine::LoadState: sync every chain at `sample_rate`, then load (the engine may have another shard count than the saver)"""
        blob = bytes(blob)
        _err(lib().gdgh_engine_load_state(self._h, blob, len(blob), sample_rate))

    def shard_range(self, shard):
        first, count = C.c_int(0), C.c_int(0)
        lib().gdgh_engine_shard_range(self._h, shard, C.byref(first), C.byref(count))
        return first.value, count.value

    def raw_context(self, shard=0):
        """the shard's gdg_ctx handle (for configuring what the twin has no class for: metronome, meters) wrapped as a package Context
        that does NOT own it"""
        import __graft_entry__ as entry
        pkg = entry.load_package()
        ctx = pkg.Context.__new__(pkg.Context)
        ctx._h = C.c_void_p(lib().gdgh_engine_context(self._h, shard))
        ctx.n_channels = self.shard_range(shard)[1]
        ctx.max_frames, ctx.device, ctx._chains = 8192, 0, []
        ctx.close = lambda: None                      # the engine owns the context
        return ctx

    def _fetch(self, kind):
        """Engine::LastBatch<kind> -> the last batch call's records of that kind, in the shape and dtype RECORD_KINDS gives it"""
        row = RECORD_KINDS[kind]
        fn = getattr(lib(), row.getter)
        n = [t(0) for t in row.counts]
        _err(fn(self._h, None, 0, *[C.byref(v) for v in n]))
        dtype = np.float64
        if row.dtype != "float64":
            import __graft_entry__ as entry
            dtype = getattr(entry.load_package(), row.dtype)
        out = np.zeros(row.shape(*[v.value for v in n]), dtype=dtype)
        _err(fn(self._h, out.ctypes.data if out.size else None, out.size, *[C.byref(v) for v in n]))
        return out

    def _set_spectrum(self, edges):
        """Engine::SetBatchSpectrum, from the `spectrum` argument of the batch calls: the band edges in Hz (None: off)"""
        self.last_spectrum = None
        if edges is None or len(edges) == 0:
            _err(lib().gdgh_engine_set_batch_spectrum(self._h, None, 0))
            return
        e = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
        _err(lib().gdgh_engine_set_batch_spectrum(self._h, e.ctypes.data, e.size))

    def _set_true_peak(self, true_peak):
        """Engine::SetBatchTruePeak, from the `true_peak` argument of the batch calls"""
        self.last_true_peak = None
        lib().gdgh_engine_set_batch_true_peak(self._h, int(bool(true_peak)))
        return bool(true_peak)

    def _set_align(self, align):
        """Engine::SetBatchAlign, from the `align` argument of the batch calls: (ref over the job's N + 3 ports, max_lag) (None: off)"""
        self.last_align = None
        if align is None or align[0] is None or len(align[0]) == 0:
            _err(lib().gdgh_engine_set_batch_align(self._h, None, 0, 0))
            return False
        ref = np.ascontiguousarray(align[0], dtype=np.int32).reshape(-1)
        _err(lib().gdgh_engine_set_batch_align(self._h, ref.ctypes.data, ref.size, int(align[1])))
        return True

    def batch_set_sources(self, source):
        """Engine::SetBatchSources: the source map of the next jobs in JOB channel numbers (None clears it); a reader whose root lives on
        another shard is refused."""
        if source is None or len(source) == 0:
            _err(lib().gdgh_engine_set_batch_sources(self._h, None, 0))
            return
        arr = (C.c_int * len(source))(*[int(v) for v in source])
        _err(lib().gdgh_engine_set_batch_sources(self._h, arr, len(source)))

    def _set_dither(self, seed):
        """Engine::SetBatchDither, from the `dither` argument of the batch calls: TPDF dither of the job's LPCM outputs with this seed
        (None: off); every shard gets its port_base from the engine, so the files do not depend on the shard count."""
        lib().gdgh_engine_set_batch_dither(self._h, 0 if seed is None else 1, 0 if seed is None else int(seed))

    def _set_delivery(self, deliver):
        """Engine::SetBatchDelivery, from the `deliver` argument of the batch calls: None or 1 = the session rate, 2 or 4 = every output at a
        half or a quarter of it, (factor, up, down) = at (rate / factor) * up / down -- delivery_for(session, delivered) finds the triple
        (one-shard engines only).  Returns the (factor, up, down) in force."""
        if isinstance(deliver, (tuple, list)):
            factor, up, down = (int(v) for v in deliver)
            _err(lib().gdgh_engine_set_batch_delivery_ratio(self._h, factor, up, down))
        else:
            _err(lib().gdgh_engine_set_batch_delivery(self._h, 1 if deliver is None else int(deliver)))
        up, down = C.c_int(1), C.c_int(1)
        lib().gdgh_engine_batch_delivery_ratio(self._h, C.byref(up), C.byref(down))
        return int(lib().gdgh_engine_batch_delivery(self._h)), up.value, down.value

    def _set_trim(self, trim):
        """Engine::SetBatchTrim, from the `trim` argument of the batch calls: the gains of the job's N + 3 output ports in the files' order
        (N chain outputs, master left, master right, metronome), or None: off.  Every shard gets its slice of the chain gains, the finishing
        context the master's."""
        if trim is None:
            _err(lib().gdgh_engine_set_batch_trim(self._h, None, 0, 1.0, 1.0, 1.0))
            return
        g = np.ascontiguousarray(trim, dtype=np.float64).reshape(-1)
        if g.size != self.n_channels + 3:
            raise HostError("trim: %d gains for the job's %d ports" % (g.size, self.n_channels + 3))
        n = self.n_channels
        _err(lib().gdgh_engine_set_batch_trim(self._h, g.ctypes.data, n, float(g[n]), float(g[n + 1]), float(g[n + 2])))

    def _set_blends(self, blends, blend_gain=None):
        """Engine::SetBatchBlends, from the `blends` / `blend_gain` arguments of the batch calls: a list of lists of (job channel, weight),
        (job channel, weight, delay in samples) or (job channel, weight, delay, taps) -- the term's FIR, up to 64 taps -- and one output
        gain per blend (None: all 1); None or an empty list: off.  Returns the number
        of blends in force: the calls' outputs and records then have N + 3 + B ports.  Refused on an engine of more than one shard."""
        blends = [] if blends is None else [list(b) for b in blends]
        if not blends:
            _err(lib().gdgh_engine_set_batch_blends(self._h, 0, None, None, None, None))
            return 0
        first = np.zeros(len(blends) + 1, dtype=np.int32)
        first[1:] = np.cumsum([len(b) for b in blends], dtype=np.int64)
        terms = [t for b in blends for t in b]
        channel = np.array([int(t[0]) for t in terms] + [0], dtype=np.int32)          # a spare entry: a list without terms still has an address
        weight = np.array([float(t[1]) for t in terms] + [0.0], dtype=np.float64)
        g = None if blend_gain is None else np.ascontiguousarray(blend_gain, dtype=np.float64).reshape(-1)
        if g is not None and g.size != len(blends):
            raise HostError("blend_gain: %d gains for %d blends" % (g.size, len(blends)))
        if any(len(t) > 3 for t in terms):
            delay = np.array([int(t[2]) if len(t) > 2 else 0 for t in terms] + [0], dtype=np.int32)
            taps =[np.asarray(t[3], dtype=np.float64).reshape(-1) if len(t) > 3 and t[3] is not None else np.zeros(0) for t in terms]
            tap_first = np.zeros(len(terms) + 1, dtype=np.int32)
            tap_first[1:] = np.cumsum([h.size for h in taps], dtype=np.int64)
            tap = np.ascontiguousarray(np.concatenate(taps + [np.zeros(1)]), dtype=np.float64)
            _err(lib().gdgh_engine_set_batch_blends_filtered(self._h, len(blends), first.ctypes.data, channel.ctypes.data, weight.ctypes.data, delay.ctypes.data,
                                                             tap_first.ctypes.data, tap.ctypes.data, None if g is None else g.ctypes.data))
            return int(lib().gdgh_engine_batch_blends(self._h))
        if any(len(t) > 2 for t in terms):
            delay = np.array([int(t[2]) if len(t) > 2 else 0 for t in terms] + [0], dtype=np.int32)
            _err(lib().gdgh_engine_set_batch_blends_delayed(self._h, len(blends), first.ctypes.data, channel.ctypes.data, weight.ctypes.data, delay.ctypes.data,
                                                            None if g is None else g.ctypes.data))
            return int(lib().gdgh_engine_batch_blends(self._h))
        _err(lib().gdgh_engine_set_batch_blends(self._h, len(blends), first.ctypes.data, channel.ctypes.data, weight.ctypes.data, None if g is None else g.ctypes.data))
        return int(lib().gdgh_engine_batch_blends(self._h))

    def _set_fits(self, fits):
        """Engine::SetBatchFits, from the `fits` argument of the batch calls: a list of (target port, [term ports]); None or an empty list:
        off.  Returns the number of fits in force.  Refused on an engine of more than one shard."""
        import __graft_entry__ as entry
        pkg = entry.load_package()
        self.last_fit = None
        fits = [] if fits is None else list(fits)
        if not fits:
            _err(lib().gdgh_engine_set_batch_fits(self._h, 0, None, None, None))
            return 0
        first, port, target = pkg._fit_csr(fits)
        _err(lib().gdgh_engine_set_batch_fits(self._h, len(fits), first.ctypes.data, port.ctypes.data, target.ctypes.data))
        return int(lib().gdgh_engine_batch_fits(self._h))

    def _set_gram(self, gram):
        """Engine::SetBatchGram, from the `gram` argument of the batch calls: a list of 2 to 512 different ports; None or an empty list: off.
        Returns the number of ports in force.  Refused on an engine of more than one shard."""
        self.last_gram = None
        ports = np.array([] if gram is None else [int(p) for p in gram], dtype=np.int32)
        _err(lib().gdgh_engine_set_batch_gram(self._h, ports.ctypes.data if ports.size else None, ports.size))
        return int(lib().gdgh_engine_batch_gram_ports(self._h))

    def _set_tapfits(self, tapfits):
        """Engine::SetBatchTapFits, from the `tapfits` argument of the batch calls: a list of (target port, [term ports], taps); None or an
        empty list: off.  Returns the number of tap fits in force.  Refused on an engine of more than one shard."""
        import __graft_entry__ as entry
        pkg = entry.load_package()
        self.last_tapfit = None
        fits = [] if tapfits is None else list(tapfits)
        if not fits:
            _err(lib().gdgh_engine_set_batch_tapfits(self._h, 0, None, None, None, None))
            return 0
        first, port, target, taps = pkg._tapfit_csr(fits)
        _err(lib().gdgh_engine_set_batch_tapfits(self._h, len(fits), first.ctypes.data, port.ctypes.data, target.ctypes.data, taps.ctypes.data))
        return int(lib().gdgh_engine_batch_tapfits(self._h))

    def _set_transfers(self, transfers):
        """Engine::SetBatchTransfers, from the `transfers` argument of the batch calls: ([(port, target), ...], group), or a list of pairs
        alone (group 1); None or an empty list: off.  Returns the number of pairs in force.  Refused on an engine of more than one shard."""
        self.last_transfer = None
        pairs, group = [], 1
        if transfers:
            if len(transfers) == 2 and np.isscalar(transfers[1]) and not np.isscalar(transfers[0]):
                pairs, group = list(transfers[0]), int(transfers[1])
            else:
                pairs = list(transfers)
        if not pairs:
            _err(lib().gdgh_engine_set_batch_transfers(self._h, 0, None, None, 1))
            return 0
        port = np.array([int(p) for p, _ in pairs] + [0], dtype=np.int32)
        target = np.array([int(t) for _, t in pairs] + [0], dtype=np.int32)
        _err(lib().gdgh_engine_set_batch_transfers(self._h, len(pairs), port.ctypes.data, target.ctypes.data, group))
        return int(lib().gdgh_engine_batch_transfers(self._h))

    def _set_loudness(self, loudness):
        """Engine::SetBatchLoudness, from the `loudness` argument of the batch calls: keep the hop records of the K-weighted session-rate rows.
        Returns whether they are on.  Refused on an engine of more than one shard."""
        self.last_loudness = None
        _err(lib().gdgh_engine_set_batch_loudness(self._h, int(bool(loudness))))
        return bool(loudness)

    def _fetch_loudness(self):
        """Engine::LastBatchLoudness: the [ports, hops] hop sums of the last batch call or slice"""
        ports, hops = C.c_int(0), C.c_size_t(0)
        _err(lib().gdgh_engine_last_batch_loudness(self._h, None, 0, C.byref(ports), C.byref(hops)))
        out = np.zeros((ports.value, hops.value), dtype=np.float64)
        _err(lib().gdgh_engine_last_batch_loudness(self._h, out.ctypes.data if out.size else None, out.size, C.byref(ports), C.byref(hops)))
        return out

    def _set_delivered(self, delivered):
        """Engine::SetBatchDelivered, from the `delivered` argument of the batch calls: keep the records of the rows the encoders read (the
        delivered rows, in front of the gains).  Returns whether they are on.  Refused on an engine of more than one shard."""
        self.last_delivered = None
        _err(lib().gdgh_engine_set_batch_delivered(self._h, int(bool(delivered))))
        return bool(delivered)

    def match_ir(self, port, target, taps, inputs, target_rate, out_format, group=32, ridge=0.0, center=0, window=16, sample_rate=None, **kw):
        """The match filter of one pass over a job: the `taps`-tap impulse response that, applied to port `port`, comes closest to port
        `target` over the whole band.  save_state; one pass with every output skipped and the one transfer pair (port, target) at group
        width `group` on; the planner (match_taps_from_transfer, with `ridge` and `center`) turns the summed records into taps; load_state:
        the engine is left as it was found.  Returns (taps [taps] float64, coherence): the taps go into ImpulseResponses.add or
        unit_set_fir like any impulse response; a response centred at `center` lags by that many samples.  Pass 1's records stay in
        match_records.  kw: batch_run's other arguments (transfers and skip_outputs in kw are replaced)."""
        import __graft_entry__ as entry
        pkg = entry.load_package()
        rate = target_rate if sample_rate is None else sample_rate
        _err(lib().gdgh_engine_sync_chains(self._h, rate))     # an engine that has not processed yet: the state to save exists from here on
        blob = self.save_state()
        rest = {k: v for k, v in kw.items() if k not in ("transfers", "skip_outputs")}
        try:
            self.batch_run(inputs, target_rate, out_format, window=window, transfers=([(int(port), int(target))], int(group)), skip_outputs=True, **rest)
            self.match_records = self.last_transfer
            h, coherence = pkg.match_taps_from_transfer(self.match_records, 1, int(group), int(taps), int(center), float(ridge))
        finally:
            self.load_state(blob, rate)
            self._set_transfers(None)
        return h[0], float(coherence[0])

    def render_tap_fitted(self, target, terms, taps, inputs, target_rate, out_format, ridge=0.0, delays=None, signs=None, center=None, window=16, sample_rate=None, **kw):
        """Two passes over one job: the `taps`-tap filters on the chain outputs `terms` (job channels, 1 to 4, terms x taps <= 128) whose sum
        comes closest to port `target` in the least-squares sense.  save_state; pass 1 renders with every output skipped and one tap fit
        on.  A term with a delay d_k or a sign (one per term, as render_aligned returns them) is measured as the port of a one-term blend
        that delays it and turns its polarity, else as the chain port itself.  The target is measured as the port of a one-term blend
        that delays it by `center` samples (default taps // 2; the target is then a chain output) -- which is what allows taps on both sides
        of the peak; center = 0 measures the target port itself (any of the N + 3 ports).  The planner (blend_taps_from_tapfit, with
        `ridge`) turns the records into taps; load_state; pass 2 renders with the one blend of the terms (channel_k, sign_k, d_k, h_k).
        THE BLEND PORT LAGS THE TARGET BY `center` SAMPLES: it approximates target[i - center].  A reach d_k + taps - 1 above 4096 is a
        HostError that names the term.  Returns (outs, taps, residual): the N + 3 + 1 output data sections, the fitted taps [terms, taps]
        and the share of the (delayed) target's energy the blend leaves.  Pass 1's records stay in tap_fitted_records.  kw: batch_run's
        other arguments (tapfits, blends and blend_gain in kw are replaced)."""
        import __graft_entry__ as entry
        pkg = entry.load_package()
        terms = [int(c) for c in terms]
        K, T, n3, N = len(terms), int(taps), self.n_channels + 3, self.n_channels
        if not 1 <= K <= pkg.TAPFIT_MAX_TERMS or not 1 <= T <= pkg.BLEND_MAX_TAPS or K * T > pkg.TAPFIT_MAX_UNKNOWNS:
            raise HostError("render_tap_fitted: %d terms (1 to %d) of %d taps (1 to %d); at most %d unknowns" % (K, pkg.TAPFIT_MAX_TERMS, T, pkg.BLEND_MAX_TAPS, pkg.TAPFIT_MAX_UNKNOWNS))
        if not 0 <= int(target) < n3:
            raise HostError("render_tap_fitted: the target is port %d; the job has ports 0 to %d" % (target, n3 - 1))
        center = T // 2 if center is None else int(center)
        if not 0 <= center <= pkg.BLEND_MAX_DELAY:
            raise HostError("render_tap_fitted: center = %d; 0 to %d" % (center, pkg.BLEND_MAX_DELAY))
        if center and int(target) >= N:
            raise HostError("render_tap_fitted: the target is port %d and center = %d: only a chain output (ports 0 to %d) can be delayed; pass center=0" % (target, center, N - 1))
        delays = [0] * K if delays is None else [int(d) for d in delays]
        signs = [1] * K if signs is None else [int(g) for g in signs]
        if len(delays) != K or len(signs) != K or any(g not in (1, -1) for g in signs) or any(d < 0 for d in delays):
            raise HostError("render_tap_fitted: one delay (>= 0) and one sign (+1 or -1) per term")
        for k in range(K):
            if delays[k] + T - 1 > pkg.BLEND_MAX_DELAY:
                raise HostError("render_tap_fitted: term %d reaches %d + %d - 1 = %d samples back; at most %d" % (k, delays[k], T, delays[k] + T - 1, pkg.BLEND_MAX_DELAY))
        rate = target_rate if sample_rate is None else sample_rate
        _err(lib().gdgh_engine_sync_chains(self._h, rate))     # an engine that has not processed yet: the state to save exists from here on
        blob = self.save_state()
        rest = {k: v for k, v in kw.items() if k not in ("tapfits", "blends", "blend_gain", "skip_outputs")}
        first, ports = [], []
        for k, c in enumerate(terms):                          # a shaped term goes through a one-term blend: ports N + 3 + ...
            if delays[k] or signs[k] != 1:
                ports.append(n3 + len(first))
                first.append([(c, float(signs[k]), delays[k])])
            else:
                ports.append(c)
        t_port = int(target)
        if center:
            t_port = n3 + len(first)
            first.append([(int(target), 1.0, center)])
        self.batch_run(inputs, target_rate, out_format, window=window, blends=first or None, tapfits=[(t_port, ports, T)], skip_outputs=True, **rest)
        self.tap_fitted_records = self.last_tapfit
        h, residual = pkg.blend_taps_from_tapfit(self.tap_fitted_records, [(t_port, ports, T)], ridge)
        self.load_state(blob, rate)
        blend = [[(c, float(signs[k]), delays[k], h[0][k]) for k, c in enumerate(terms)]]
        outs = self.batch_run(inputs, target_rate, out_format, window=window, blends=blend, **rest)
        return outs, h[0], float(residual[0])

    def render_matched(self, target, candidates, max_terms, inputs, target_rate, out_format, ridge=0.0, min_gain=0.0, window=16, sample_rate=None, **kw):
        """Two passes over one job: which few of `candidates`, in which mix, come closest to port `target` (a chain output, master left,
        master right or the metronome).  A candidate is a job channel, or (job channel, delay, sign) -- then it is measured as the port of a
        one-term blend that delays it and turns its polarity, as in render_fitted.  save_state; pass 1 renders with every output skipped and
        the Gram list [target] + candidates on; the planner (blend_pick_from_gram) picks up to max_terms of them greedily; load_state;
        pass 2 renders with the one blend of the picked candidates at weights sign * w and their delays.  Returns (outs, picked, weights,
        residuals): the N + 3 + 1 output data sections (N + 3 when nothing was picked), the positions in `candidates` in pick order, the
        weights as fitted (before the signs) and the share of the target's energy left after every pick.  Pass 1's records stay in
        matched_records.  kw: batch_run's other arguments (gram, fits, blends and blend_gain in kw are replaced)."""
        import __graft_entry__ as entry
        pkg = entry.load_package()
        n3 = self.n_channels + 3
        cands = [(int(c), 0, 1) if np.isscalar(c) else (int(c[0]), int(c[1]), int(c[2])) for c in candidates]
        if not 1 <= len(cands) <= pkg.GRAM_MAX_PORTS - 1:
            raise HostError("render_matched: %d candidates; 1 to %d" % (len(cands), pkg.GRAM_MAX_PORTS - 1))
        if not 0 <= int(target) < n3:
            raise HostError("render_matched: the target is port %d; the job has ports 0 to %d" % (target, n3 - 1))
        if any(g not in (1, -1) for _, _, g in cands):
            raise HostError("render_matched: a candidate's sign is +1 or -1")
        rate = target_rate if sample_rate is None else sample_rate
        _err(lib().gdgh_engine_sync_chains(self._h, rate))     # an engine that has not processed yet: the state to save exists from here on
        blob = self.save_state()
        rest = {k: v for k, v in kw.items() if k not in ("gram", "fits", "blends", "blend_gain", "skip_outputs")}
        shaped = [k for k, (_, d, g) in enumerate(cands) if d or g != 1]       # these go through a one-term blend each: ports N + 3 + ...
        first = [[(cands[k][0], float(cands[k][2]), cands[k][1])] for k in shaped]
        ports = [n3 + shaped.index(k) if k in shaped else cands[k][0] for k in range(len(cands))]
        self.batch_run(inputs, target_rate, out_format, window=window, blends=first or None, gram=[int(target)] + ports, skip_outputs=True, **rest)
        self.matched_records = self.last_gram
        picked, weights, residuals = pkg.blend_pick_from_gram(self.matched_records, 1 + len(cands), 0, list(range(1, 1 + len(cands))), max_terms, ridge, min_gain)
        picked = [p - 1 for p in picked]
        self.load_state(blob, rate)
        blend = [[(cands[k][0], cands[k][2] * float(w), cands[k][1]) for k, w in zip(picked, weights)]] if picked else None
        outs = self.batch_run(inputs, target_rate, out_format, window=window, blends=blend, **rest)
        return outs, picked, [float(w) for w in weights], [float(r) for r in residuals]

    def render_fitted(self, target, terms, inputs, target_rate, out_format, ridge=0.0, delays=None, signs=None, window=16, sample_rate=None, **kw):
        """Two passes over one job: the blend of the chain outputs `terms` (job channels, 1 to 8) that comes closest to port `target` (a chain
        output, master left, master right or the metronome) in the least-squares sense.  save_state; pass 1 renders with every output
        skipped and one fit on: against `target`, each term the chain port itself -- or, with delays and / or signs given (one per term, as
        render_aligned returns them), the port of a one-term blend that delays it and turns its polarity; the planner
        (blend_weights_from_fit) turns the records into weights; load_state; pass 2 renders with the one blend of weights sign_k * w_k and
        the given delays.  Returns (outs, weights, residual): the N + 3 + 1 output data sections, the K weights as fitted (before the
        signs) and the share of the target's energy the blend leaves.  Pass 1's records stay in fitted_records.  kw: batch_run's other
        arguments (fits, blends and blend_gain in kw are replaced)."""
        import __graft_entry__ as entry
        pkg = entry.load_package()
        terms = [int(c) for c in terms]
        K, n3 = len(terms), self.n_channels + 3
        if not 1 <= K <= pkg.FIT_MAX_TERMS:
            raise HostError("render_fitted: %d terms; 1 to %d" % (K, pkg.FIT_MAX_TERMS))
        if not 0 <= int(target) < n3:
            raise HostError("render_fitted: the target is port %d; the job has ports 0 to %d" % (target, n3 - 1))
        delays = [0] * K if delays is None else [int(d) for d in delays]
        signs = [1] * K if signs is None else [int(g) for g in signs]
        if len(delays) != K or len(signs) != K or any(g not in (1, -1) for g in signs):
            raise HostError("render_fitted: one delay and one sign (+1 or -1) per term")
        shaped = any(delays) or any(g != 1 for g in signs)
        rate = target_rate if sample_rate is None else sample_rate
        _err(lib().gdgh_engine_sync_chains(self._h, rate))     # an engine that has not processed yet: the state to save exists from here on
        blob = self.save_state()
        rest = {k: v for k, v in kw.items() if k not in ("fits", "blends", "blend_gain", "skip_outputs")}
        if shaped:                                           # term k as blend port N + 3 + k: delayed and turned before it is measured
            first = [[(c, float(signs[k]), delays[k])] for k, c in enumerate(terms)]
            self.batch_run(inputs, target_rate, out_format, window=window, blends=first, fits=[(int(target), [n3 + k for k in range(K)])], skip_outputs=True, **rest)
        else:
            self.batch_run(inputs, target_rate, out_format, window=window, fits=[(int(target), terms)], skip_outputs=True, **rest)
        self.fitted_records = self.last_fit
        weight, residual = pkg.blend_weights_from_fit(self.fitted_records, ridge)
        weights = [float(w) for w in weight[0, :K]]
        self.load_state(blob, rate)
        blend = [[(c, signs[k] * weights[k], delays[k]) for k, c in enumerate(terms)]]
        outs = self.batch_run(inputs, target_rate, out_format, window=window, blends=blend, **rest)
        return outs, weights, float(residual[0])

    def render_aligned(self, blends, max_lag, min_coeff, inputs, target_rate, out_format, window=16, sample_rate=None, fraction_steps=0, fraction_taps=32, **kw):
        """Two passes over one job: the terms of every blend are lined up before they are summed.  save_state; pass 1 renders with every
        output skipped and the alignment records on, every term's channel measured against the channel of its blend's first term (a channel
        that two blends measure against different first terms is refused); the planner (blend_delays_from_align) turns the records into
        one delay and one sign per term; load_state; pass 2 renders with the delayed blends, the weights multiplied by the signs.  blends:
        lists of (job channel, weight).  Returns (outs, delays, signs): the N + 3 + B output data sections, and per blend the list of delays
        and of signs used.  Pass 1's records stay in aligned_records.  kw: batch_run's other arguments (an align in kw is replaced).
        fraction_steps = Q > 0 (1 to 4) lines the terms up to 1/Q of a sample: a pass between the planner and the render gives every
        measured channel 2Q - 1 one-term filtered blend ports around its whole-sample plan -- candidate `step` of -(Q - 1) .. Q - 1 delays by
        n samples and fraction_taps windowed-sinc taps for f (blend_fraction_taps), n + f = d + 1 + step / Q -- and its blend's first term
        one port delayed by the common latency, d + fraction_taps / 2; one fit per measured channel against that port, every output
        skipped; blend_fractions_from_fit picks the step, and the last pass renders with it.  Every term of such a blend ends
        fraction_taps / 2 samples later than the whole-sample plan put it -- a term without taps gets d + fraction_taps / 2 --, so the
        blend port LAGS the chain ports by fraction_taps / 2 samples.  A plan that reaches further back than 4096 samples is a HostError
        that names the blend.  Returns (outs, delays, signs, fractions) in this mode: fractions[b][k] = step / Q of term k, 0.0 for a term
        that was not measured; the pass's records stay in fraction_records.  fraction_steps = 0: exactly the two passes above."""
        import __graft_entry__ as entry
        pkg = entry.load_package()
        Q, T = int(fraction_steps), int(fraction_taps)
        if Q < 0 or Q > 4 or (Q > 0 and (T < 2 or T > pkg.BLEND_MAX_TAPS or T % 2)):
            raise HostError("render_aligned: fraction_steps = %d (0 to 4), fraction_taps = %d (even, 2 to %d)" % (Q, T, pkg.BLEND_MAX_TAPS))
        blends = [[(int(t[0]), float(t[1])) for t in b] for b in blends]
        n3 = self.n_channels + 3
        ref = [-1] * n3
        for b, terms in enumerate(blends):
            root = terms[0][0]
            for c, _ in terms:
                if c == root:
                    continue
                if ref[c] not in (-1, root):
                    raise HostError("render_aligned: channel %d is measured against channel %d and, in blend %d, against channel %d" % (c, ref[c], b, root))
                ref[c] = root
        for b, terms in enumerate(blends):                      # a first term that another blend measures against something else
            if ref[terms[0][0]] != -1 and any(c != terms[0][0] for c, _ in terms):
                raise HostError("render_aligned: blend %d's first term, channel %d, is measured against channel %d in another blend" % (b, terms[0][0], ref[terms[0][0]]))
        rate = target_rate if sample_rate is None else sample_rate
        _err(lib().gdgh_engine_sync_chains(self._h, rate))     # an engine that has not processed yet: the state to save exists from here on
        blob = self.save_state()
        rest = {k: v for k, v in kw.items() if k not in ("align", "blends", "skip_outputs")}
        self.batch_run(inputs, target_rate, out_format, window=window, align=(ref, max_lag), skip_outputs=True, **rest)
        self.aligned_records = self.last_align
        delays, signs = pkg.blend_delays_from_align(self.aligned_records, ref, blends, min_coeff)
        self.load_state(blob, rate)
        if Q > 0:
            return self._render_fractions(pkg, blends, delays, signs, ref, Q, T, blob, rate, inputs, target_rate, out_format, window, rest)
        lined = [[(c, w * signs[b][k], delays[b][k]) for k, (c, w) in enumerate(terms)] for b, terms in enumerate(blends)]
        outs = self.batch_run(inputs, target_rate, out_format, window=window, blends=lined, **rest)
        return outs, delays, signs

    def _render_fractions(self, pkg, blends, delays, signs, ref, Q, T, blob, rate, inputs, target_rate, out_format, window, rest):
        """render_aligned's pass between the planner and the render, and the render: see there"""
        n3 = self.n_channels + 3

        def filtered(c, w, d, step):                          # n + f = d + 1 + step / Q, in whole Q-ths
            num = (d + 1) * Q + step
            return (c, w, num // Q, pkg.blend_fraction_taps(T, (num % Q) / float(Q)))

        def reach_ok(b, term):
            d, taps = term[2], term[3] if len(term) > 3 else ()
            if d + max(len(taps), 1) - 1 > pkg.BLEND_MAX_DELAY:
                raise HostError("render_aligned: blend %d: channel %d would be read %d samples back with %d taps; a term reaches at most %d samples"
                                % (b, term[0], d, len(taps), pkg.BLEND_MAX_DELAY))
            return term

        # the ports of the pass: per root one, per measured channel 2Q - 1, planned in the first blend that holds the channel
        ports, root_port, fits, measured = [], {}, [], []
        for b, terms in enumerate(blends):
            root = terms[0][0]
            for k, (c, _) in enumerate(terms):
                if c == root or c in measured:
                    continue
                if (b, root) not in root_port:
                    root_port[(b, root)] = n3 + len(ports)
                    ports.append([reach_ok(b, (root, 1.0, delays[b][0] + T // 2))])
                cand = []
                for step in range(-(Q - 1), Q):
                    cand.append(n3 + len(ports))
                    ports.append([reach_ok(b, filtered(c, float(signs[b][k]), delays[b][k], step))])
                fits.append((root_port[(b, root)], cand))
                measured.append(c)
        steps = {}
        if fits:
            self.batch_run(inputs, target_rate, out_format, window=window, blends=ports, fits=fits, skip_outputs=True,
                           **{k: v for k, v in rest.items() if k not in ("fits", "blend_gain")})
            self.fraction_records = self.last_fit
            steps = dict(zip(measured, pkg.blend_fractions_from_fit(self.fraction_records, Q)))
            self.load_state(blob, rate)
        lined, fractions = [], []
        for b, terms in enumerate(blends):
            lined.append([reach_ok(b, filtered(c, w * signs[b][k], delays[b][k], steps[c]) if c in steps and c != terms[0][0] else (c, w * signs[b][k], delays[b][k] + T // 2))
                          for k, (c, w) in enumerate(terms)])
            fractions.append([steps[c] / float(Q) if c in steps and c != terms[0][0] else 0.0 for c, _ in terms])
        outs = self.batch_run(inputs, target_rate, out_format, window=window, blends=lined, **rest)
        return outs, delays, signs, fractions

    def render_normalized(self, target_dbtp, max_gain_db, inputs, target_rate, out_format, window=16, sample_rate=None, measure="render", target_lufs=-23.0,
                          ceiling_dbtp=None, **kw):
        """Two passes over one job: every output file is written with the gain that brings its true peak to target_dbtp (dBTP), capped at
        max_gain_db.  save_state; pass 1 renders with the true-peak records (and the report) on and every output skipped; the planner
        (trim_from_true_peak) turns the records into gains; load_state; pass 2 renders with the trim.  Returns (outs, gains): the N + 3
        output data sections and the N + 3 gains used -- with blends= in kw N + 3 + B of each: a blend port's gain is planned from its own
        true-peak records like any other port's and passed as its output gain (a blend_gain in kw is replaced).  The master's gains come from the finish's own records of pass 1, whatever the
        shard count.  Pass 1's records stay in normalize_true_peak / normalize_report.  The state blob is the channels': a configured
        metronome and the meters run on from pass 1.  kw: batch_run's other arguments (dither, run_meters ...).  deliver= is carried through
        both passes unchanged.  measure="render" (the default): the gains are planned from the session-rate records, and a delivered file's
        true peak can differ from the render's (the anti-aliasing filter rings), so leave the headroom the target is meant to leave.
        measure="delivered" (one-shard engines): pass 1 runs with the delivery in force and the records of the delivered rows on; the
        planner (trim_from_delivered) takes their true peak -- that of the rows the files are encoded from, seamless across blocks -- and
        the records stay in normalize_delivered: a file normalised to -1 dBTP then measures -1 dBTP.
        measure="loudness" (one-shard engines): pass 1 runs with the loudness records (include/gdg.h, LOUDNESS) on; the planner
        (trim_from_loudness) brings every port's own integrated loudness to target_lufs and caps a gain that would carry the port's true peak
        over ceiling_dbtp (None: target_dbtp); max_gain_db caps it as well.  The records stay in normalize_loudness, and normalize_capped says
        which ports the ceiling capped.  The records are of the session-rate render: with a delivery factor in force the file is quieter by the
        decimator's attenuation (ATTENUATION_HALF_DECIBEL, once whatever the factor), so the plan adds that constant back."""
        if measure not in ("render", "delivered", "loudness"):
            raise ValueError("measure: 'render', 'delivered' or 'loudness'")
        import __graft_entry__ as entry
        pkg = entry.load_package()
        rate = target_rate if sample_rate is None else sample_rate
        _err(lib().gdgh_engine_sync_chains(self._h, rate))     # an engine that has not processed yet: the state to save exists from here on
        blob = self.save_state()
        self.batch_run(inputs, target_rate, out_format, window=window, report=True, true_peak=True, skip_outputs=True, delivered=measure == "delivered",
                       loudness=measure == "loudness", **{k: v for k, v in kw.items() if k not in ("report", "true_peak", "trim", "blend_gain", "delivered", "loudness")})
        self.normalize_true_peak, self.normalize_report = self.last_true_peak, self.last_report
        if measure == "delivered":
            self.normalize_delivered = self.last_delivered
            gains = pkg.trim_from_delivered(self.normalize_delivered, 10.0 ** (target_dbtp / 20.0), 10.0 ** (max_gain_db / 20.0))
        elif measure == "loudness":
            self.normalize_loudness = self.last_loudness
            deliver = kw.get("deliver")
            factor = deliver[0] if isinstance(deliver, (tuple, list)) else (deliver or 1)
            back = -20.0 * math.log10(ATTENUATION_HALF_DECIBEL) if int(factor) > 1 else 0.0      # what the factor's decimator takes from the file
            gains, self.normalize_capped = pkg.trim_from_loudness(self.normalize_loudness, target_rate, target_lufs + back,
                                                                  target_dbtp if ceiling_dbtp is None else ceiling_dbtp, self.normalize_true_peak)
            gains = np.minimum(gains, 10.0 ** (max_gain_db / 20.0))
        else:
            gains = pkg.trim_from_true_peak(self.normalize_true_peak, 10.0 ** (target_dbtp / 20.0), 10.0 ** (max_gain_db / 20.0))
        self.load_state(blob, rate)
        n3 = self.n_channels + 3                              # the trim's ports; the gains behind them are the blend ports'
        outs = self.batch_run(inputs, target_rate, out_format, window=window, trim=gains[:n3], blend_gain=gains[n3:] if gains.size > n3 else None,
                              **{k: v for k, v in kw.items() if k not in ("trim", "blend_gain")})
        return outs, gains

    def batch_run(self, inputs, target_rate, out_format, window=16, metronome_to_master=False, run_meters=False, tuner_enqueue=False,
                  report=False, dither=None, spectrum=None, align=None, true_peak=False, trim=None, skip_outputs=False, blends=None, blend_gain=None, fits=None, gram=None, tapfits=None, transfers=None, deliver=None, delivered=False, loudness=False):
        """Engine::BatchRun: controller.processFiles' data path over all shards; returns the N + 3 output data sections.  report: keep the
        render report of the run in last_report ([N + 3, blocks], gdg_batch_run's port order whatever the shard count).  spectrum: band
        edges in Hz -- keep the band spectrum of the run in last_spectrum ([N + 3, blocks, bands], the same order).  align: (ref, max_lag) --
        keep the alignment records in last_align ([N + 3, blocks]); over shards the master rows are zero records.  true_peak: keep the
        true-peak records in last_true_peak ([N + 3, blocks], the same order).  trim: the N + 3 gains in front of the encoders (None:
        off).  skip_outputs: every output pointer NULL -- the job renders and measures, nothing is written; returns None.  blends: a list
        of lists of (job channel, weight) or (job channel, weight, delay), blend_gain: one output gain per blend -- B more outputs and B more ports in every last_* record
        list, behind the metronome's (one-shard engines only; None: off).  fits: a list of (target port, [term ports]) -- keep the fit
        records in last_fit ([fits, blocks], FIT_DTYPE; one-shard engines only; None: off).  gram: a list of 2 to 512 different ports -- keep the
        Gram records in last_gram ([blocks, P (P + 1) / 2] float64; one-shard engines only; None: off).  tapfits: a list of (target port,
        [term ports], taps) -- keep the tap-fit records in last_tapfit ([blocks, D] float64; one-shard engines only; None: off).  transfers:
        ([(port, target), ...], group) -- keep the transfer records in last_transfer ([blocks, pairs x G x 4] float64; one-shard engines only; None: off).
        deliver: 2 or 4 -- every output at a half or a quarter of the session rate (Engine::SetBatchDelivery; one-shard engines only; None
        or 1: off): each data section then has length // deliver samples and lags the render by 38 or 77 session samples.  A triple
        (factor, up, down) -- delivery_for(192000, 44100) = (4, 147, 160) -- adds the ratio stage behind the factor: each data section has
        batch_delivery_samples(factor, up, down, 0, length) samples and lags by batch_delivery_ratio_latency(factor, up, down).  Every last_*
        record stays that of the session-rate render, so a delivered file's true peak can differ from last_true_peak: the anti-aliasing
        filter removes what lies above the new Nyquist frequency, and it rings.  delivered: keep the records of the rows the encoders read
        -- behind the delivery, in front of the trim and blend gains -- in last_delivered ([N + 3 + B, blocks], BLOCK_DELIVERED_DTYPE; one-shard
        engines only): their true_peak is the delivered file's, seamless across blocks.  loudness: keep the loudness records -- per port and
        100 ms hop the sum of squares of the K-weighted session-rate samples -- in last_loudness ([N + 3 + B, hops] float64; one-shard engines
        only); loudness_from_hops and trim_from_loudness of the package read them."""
        import __graft_entry__ as entry
        pkg = entry.load_package()
        loud = self._set_loudness(loudness)
        R, nb, kinds = self._settings(report=report, dither=dither, spectrum=spectrum, align=align, true_peak=true_peak, trim=trim, blends=blends, blend_gain=blend_gain,
                                      fits=fits, gram=gram, tapfits=tapfits, transfers=transfers, deliver=deliver, delivered=delivered)
        n = len(inputs)
        arr, _datas, _widths, opt, wo = self._job_inputs(pkg, inputs, target_rate, out_format, metronome_to_master, run_meters, tuner_enqueue)
        # the job's length: the longest shard's (asked from the shards' own contexts)
        length = 0
        for g in range(self.shards()):
            first, count = self.shard_range(g)
            if count > 0:
                length = max(length, self.raw_context(g).batch_length(inputs[first:first + count], target_rate))
        no = n + 3 + nb
        outs = None if skip_outputs else [np.zeros(pkg.batch_delivery_samples(*R, 0, length) * wo, dtype=np.uint8) for _ in range(no)]
        ptrs = (C.c_void_p * no)(*([None] * no if skip_outputs else [(o.ctypes.data if o.size else None) for o in outs]))
        samples = C.c_size_t(0)
        _err(lib().gdgh_engine_batch_run(self._h, arr, n, C.byref(opt), window, ptrs, C.byref(samples)))
        assert samples.value == length
        for kind in kinds:
            setattr(self, RECORD_KINDS[kind].attr, self._fetch(kind))
        if loud:
            self.last_loudness = self._fetch_loudness()
        return outs

    def batch_stream(self, inputs, target_rate, out_format, blocks_per_slice, window=16, metronome_to_master=False, run_meters=False, tuner_enqueue=False,
                     report=False, dither=None, spectrum=None, align=None, true_peak=False, trim=None, blends=None, blend_gain=None, fits=None, gram=None, tapfits=None, transfers=None, deliver=None, delivered=False):
        """Engine::BatchStreamOpen / Need / Step / Close over the `inputs` tuples of batch_run, `blocks_per_slice` blocks at a time:
        yields every slice's N + 3 output pieces (and one per blend of blends= / blend_gain=, as batch_run's).  report: last_report grows by every slice's records and is the whole job's,
        [N + 3, blocks], when the generator ends; spectrum=edges: last_spectrum likewise, [N + 3, blocks, bands]; fits=: last_fit likewise,
        [fits, blocks]; gram=: last_gram likewise, [blocks, P (P + 1) / 2]; tapfits=: last_tapfit likewise, [blocks, D].  deliver=: as
        batch_run's -- every piece has blocks * 8192 // deliver samples; the records stay those of the session-rate render.  delivered=True:
        last_delivered grows by every slice's records of the delivered rows, [N + 3 + B, blocks] when the generator ends."""
        L = lib()
        return self._batch_stream((L.gdgh_engine_batch_stream_open, L.gdgh_engine_batch_stream_need, L.gdgh_engine_batch_stream_step,
                                   L.gdgh_engine_batch_stream_close), inputs, target_rate, out_format, blocks_per_slice, window,
                                  metronome_to_master, run_meters, tuner_enqueue, report=report, dither=dither, spectrum=spectrum, align=align, true_peak=true_peak, trim=trim,
                                  blends=blends, blend_gain=blend_gain, fits=fits, gram=gram, tapfits=tapfits, transfers=transfers, deliver=deliver, delivered=delivered)

    def batch_stream_sharded_checkpoint(self):
        """Engine::BatchStreamShardedCheckpoint -> bytes: the open sharded job (call it between two slices of batch_stream_sharded)"""
        p, n = C.c_void_p(), C.c_size_t(0)
        _err(lib().gdgh_engine_batch_stream_sharded_checkpoint(self._h, C.byref(p), C.byref(n)))
        try:
            return C.string_at(p, n.value)
        finally:
            lib().gdgh_free(p)

    def batch_stream_sharded(self, inputs, target_rate, out_format, blocks_per_slice, window=16, metronome_to_master=False, run_meters=False,
                             tuner_enqueue=False, report=False, dither=None, resume=None, spectrum=None, align=None, true_peak=False, trim=None):
        """Engine::BatchStreamShardedOpen / Need / Step / Close: batch_stream for an engine of any shard count -- every shard streams its
        channels, the master is finished per slice; yields every slice's N + 3 output pieces (blocks_per_slice: an int or a function
        (blocks_left) -> blocks).  report: as batch_stream's -- the chain rows come from the shards, the master from the finish, the
        metronome from shard 0; spectrum=edges: last_spectrum, from the same three sources.  resume: a blob of batch_stream_sharded_checkpoint -- Engine::BatchStreamShardedResume in the place of the
        Open call (same inputs and options, set up again on this engine); the slices go on where the checkpoint was taken."""
        L = lib()
        return self._batch_stream((L.gdgh_engine_batch_stream_sharded_open, L.gdgh_engine_batch_stream_sharded_need,
                                   L.gdgh_engine_batch_stream_sharded_step, L.gdgh_engine_batch_stream_sharded_close), inputs, target_rate,
                                  out_format, blocks_per_slice, window, metronome_to_master, run_meters, tuner_enqueue, resume=resume, report=report, dither=dither,
                                  spectrum=spectrum, align=align, true_peak=true_peak, trim=trim)

    def _settings(self, report=False, dither=None, spectrum=None, align=None, true_peak=False, trim=None, blends=None, blend_gain=None, fits=None, gram=None, tapfits=None,
                  transfers=None, deliver=None, delivered=False):
        """The batch calls' settings onto the engine (Engine::SetBatch*), in the one order both calls use; every last_* a call may fill is
        None afterwards.  Returns ((factor, up, down) of the delivery in force, the blends in force, the kinds of records that are on, in
        RECORD_KINDS' order)."""
        lib().gdgh_engine_set_batch_report(self._h, int(bool(report)))
        self._set_dither(dither)
        self._set_trim(trim)
        R = self._set_delivery(deliver)
        nb = self._set_blends(blends, blend_gain)            # before the alignment list, which may name blend ports
        on = {"report": bool(report), "spectrum": spectrum is not None and len(spectrum) > 0}
        on["fit"] = self._set_fits(fits)
        on["gram"] = self._set_gram(gram)
        on["tapfit"] = self._set_tapfits(tapfits)
        on["transfer"] = self._set_transfers(transfers)
        on["delivered"] = self._set_delivered(delivered)
        self._set_spectrum(spectrum)
        on["align"] = self._set_align(align)
        on["true_peak"] = self._set_true_peak(true_peak)
        self.last_report = None
        return R, nb, [kind for kind in RECORD_KINDS if on[kind]]

    @staticmethod
    def _job_inputs(pkg, inputs, target_rate, out_format, metronome_to_master, run_meters, tuner_enqueue):
        """The `inputs` tuples (data, format, rate[, channels, channel]; None: no file) as the BatchInput array of the C calls -> (the
        array, every input's bytes (they must outlive the call), the bytes of one source frame per input, the BatchOptions, the bytes of
        one output sample)"""
        n = len(inputs)
        arr = (pkg.BatchInput * n)()
        datas, widths = [None] * n, [0] * n
        for i, it in enumerate(inputs):
            if it is None:
                continue
            channels, channel = (it[3], it[4]) if len(it) > 3 else (1, 0)
            f = pkg.WAVE_FORMATS[it[1]] if isinstance(it[1], str) else it[1]
            datas[i] = np.ascontiguousarray(it[0], dtype=np.uint8)
            widths[i] = max(pkg.lib().gdg_wave_bytes_per_sample(f), 1) * max(channels, 1)
            arr[i] = pkg.BatchInput(datas[i].ctypes.data if datas[i].size else None, datas[i].size // widths[i], f, it[2], channels, channel)
        fo = pkg.WAVE_FORMATS[out_format] if isinstance(out_format, str) else out_format
        opt = pkg.BatchOptions(target_rate, fo, int(bool(metronome_to_master)), int(bool(run_meters)), int(bool(tuner_enqueue)))
        return arr, datas, widths, opt, pkg.lib().gdg_wave_bytes_per_sample(fo)

    def _batch_stream(self, calls, inputs, target_rate, out_format, blocks_per_slice, window, metronome_to_master, run_meters, tuner_enqueue, resume=None, **settings):
        f_open, f_need, f_step, f_close = calls
        import __graft_entry__ as entry
        pkg = entry.load_package()
        R, nb, kinds = self._settings(**settings)             # the sharded form passes no delivery, no blends and none of the five list kinds: off
        n = len(inputs)
        arr, datas, widths, opt, wo = self._job_inputs(pkg, inputs, target_rate, out_format, metronome_to_master, run_meters, tuner_enqueue)
        samples, done = C.c_size_t(0), C.c_size_t(0)
        if resume is None:
            _err(f_open(self._h, arr, n, C.byref(opt), window, C.byref(samples)))
        else:                                                # the job's length as the Open call computes it: the longest shard's
            for g in range(self.shards()):
                first, count = self.shard_range(g)
                if count > 0:
                    samples.value = max(samples.value, self.raw_context(g).batch_length(inputs[first:first + count], target_rate))
            blob = bytes(resume)
            _err(lib().gdgh_engine_batch_stream_sharded_resume(self._h, arr, n, C.byref(opt), window, blob, len(blob), C.byref(done)))
        try:
            left = (samples.value - done.value) // 8192
            first, count = (C.c_size_t * n)(), (C.c_size_t * n)()
            done_samples = done.value                        # session samples of the slices so far: what a delivery ratio counts a slice from
            while left:
                blocks = min(left, blocks_per_slice(left) if callable(blocks_per_slice) else blocks_per_slice)
                _err(f_need(self._h, blocks, first, count))
                pieces = [None if datas[i] is None or not count[i] else datas[i][first[i] * widths[i]:(first[i] + count[i]) * widths[i]] for i in range(n)]
                ins = (C.c_void_p * n)(*[(p.ctypes.data if p is not None else None) for p in pieces])
                outs = [np.zeros(pkg.batch_delivery_samples(*R, done_samples, blocks * 8192) * wo, dtype=np.uint8) for _ in range(n + 3 + nb)]
                done_samples += blocks * 8192
                ptrs = (C.c_void_p * (n + 3 + nb))(*[o.ctypes.data for o in outs])
                _err(f_step(self._h, blocks, ins, ptrs))
                for kind in kinds:                           # every last_* grows by the slice's records, along the kind's block axis
                    row, rec = RECORD_KINDS[kind], self._fetch(kind)
                    setattr(self, row.attr, rec if getattr(self, row.attr) is None else np.concatenate([getattr(self, row.attr), rec], axis=row.axis))
                yield outs
                left -= blocks
        finally:
            f_close(self._h)


class Chain:
    """signal.Chain: the 14 methods of signal/signal.go:21-36."""

    def __init__(self, handle, irs):
        self._h = handle
        self._irs = irs          # keep the library alive

    def _close(self):
        if self._h:
            lib().gdgh_chain_destroy(self._h)
            self._h = None

    def AppendUnit(self, unit_type):
        i = C.c_int(-1)
        _err(lib().gdgh_chain_append_unit(self._h, unit_type, C.byref(i)))
        return i.value

    def RemoveUnit(self, i):
        _err(lib().gdgh_chain_remove_unit(self._h, i))

    def MoveUp(self, i):
        _err(lib().gdgh_chain_move_up(self._h, i))

    def MoveDown(self, i):
        _err(lib().gdgh_chain_move_down(self._h, i))

    def UnitType(self, i):
        t = C.c_int(-1)
        _err(lib().gdgh_chain_unit_type(self._h, i, C.byref(t)))
        return t.value

    def SetBypass(self, i, bypass):
        _err(lib().gdgh_chain_set_bypass(self._h, i, 1 if bypass else 0))

    def GetBypass(self, i):
        b = C.c_int(0)
        _err(lib().gdgh_chain_get_bypass(self._h, i, C.byref(b)))
        return bool(b.value)

    def SetDiscreteValue(self, i, name, value):
        _err(lib().gdgh_chain_set_discrete(self._h, i, name.encode(), value.encode()))

    def GetDiscreteValue(self, i, name):
        buf = C.create_string_buffer(512)
        _err(lib().gdgh_chain_get_discrete(self._h, i, name.encode(), buf, 512))
        return buf.value.decode()

    def SetNumericValue(self, i, name, value):
        _err(lib().gdgh_chain_set_numeric(self._h, i, name.encode(), int(value)))

    def GetNumericValue(self, i, name):
        v = C.c_int32(0)
        _err(lib().gdgh_chain_get_numeric(self._h, i, name.encode(), C.byref(v)))
        return v.value

    def Parameters(self, i):
        buf = C.create_string_buffer(1 << 16)
        _err(lib().gdgh_chain_parameters(self._h, i, buf, 1 << 16))
        out = []
        for line in buf.value.decode().splitlines():
            name, typ, unit, mn, mx, num, idx, vals = line.split("|")
            out.append({"Name": name, "Type": int(typ), "PhysicalUnit": unit, "Minimum": int(mn), "Maximum": int(mx),
                        "NumericValue": int(num), "DiscreteValueIndex": int(idx), "DiscreteValues": vals.split(";") if vals else []})
        return out

    def Length(self):
        return lib().gdgh_chain_length(self._h)

    def Process(self, x, sample_rate, n_out=None):
        x = _f64(x)
        n_out = x.size if n_out is None else n_out
        out = np.full(n_out, np.nan)
        lib().gdgh_chain_process(self._h, x.ctypes.data, x.size, out.ctypes.data, n_out, sample_rate)
        return out


class Spatializer:
    """spatializer.Spatializer: the ten methods of spatializer/spatializer.go:30-41 on top of an Engine's shards."""

    def __init__(self, engine, input_channels):
        self._engine = engine
        self._h = lib().gdgh_spatializer_create(engine._h, input_channels)

    def __del__(self):
        if getattr(self, "_h", None):
            lib().gdgh_spatializer_destroy(self._h)
            self._h = None

    def _get(self, what, ch):
        v = C.c_double(0.0)
        _err(lib().gdgh_spatializer_get(self._h, what, ch, C.byref(v)))
        return v.value

    def GetAzimuth(self, ch): return self._get(0, ch)
    def GetDistance(self, ch): return self._get(1, ch)
    def GetLevel(self, ch): return self._get(2, ch)
    def SetAzimuth(self, ch, v): _err(lib().gdgh_spatializer_set(self._h, 0, ch, float(v)))
    def SetDistance(self, ch, v): _err(lib().gdgh_spatializer_set(self._h, 1, ch, float(v)))
    def SetLevel(self, ch, v): _err(lib().gdgh_spatializer_set(self._h, 2, ch, float(v)))
    def GetInputCount(self): return lib().gdgh_spatializer_input_count(self._h)
    def GetOutputCount(self): return lib().gdgh_spatializer_output_count(self._h)
    def SetSampleRate(self, rate): lib().gdgh_spatializer_set_sample_rate(self._h, rate)

    def Process(self, x, aux=None, reuse_chain_outputs=False):
        x = _f64(x)
        n = x.shape[1]
        ins = (C.c_void_p * x.shape[0])(*[x[i].ctypes.data for i in range(x.shape[0])])
        a = _f64(aux) if aux is not None else None
        left, right = np.full(n, np.nan), np.full(n, np.nan)
        lib().gdgh_spatializer_process(self._h, ins, a.ctypes.data if a is not None else None, left.ctypes.data, right.ctypes.data, n,
                                       1 if reuse_chain_outputs else 0)
        return left, right


class Tuner:
    """tuner.Tuner (tuner/tuner.go:62-65)."""

    def __init__(self, device=0):
        self._h = lib().gdgh_tuner_create(device)

    def __del__(self):
        if getattr(self, "_h", None):
            lib().gdgh_tuner_destroy(self._h)
            self._h = None

    def Process(self, samples, sample_rate):
        s = _f64(samples)
        lib().gdgh_tuner_process(self._h, s.ctypes.data, s.size, sample_rate)

    def Analyze(self):
        cents, freq, note = C.c_int(0), C.c_double(0.0), C.create_string_buffer(64)
        _err(lib().gdgh_tuner_analyze(self._h, C.byref(cents), C.byref(freq), note, 64))
        return {"cents": cents.value, "frequency": freq.value, "note": note.value.decode()}


class Unit:
    """A stand-alone effects.Unit (runs on a private one-channel context)."""

    def __init__(self, unit_type):
        self._h = lib().gdgh_unit_create(unit_type)
        if not self._h:
            raise HostError("Failed to create effects unit.")

    def __del__(self):
        if getattr(self, "_h", None):
            lib().gdgh_unit_destroy(self._h)
            self._h = None

    def SetNumericValue(self, name, value):
        _err(lib().gdgh_unit_set_numeric(self._h, name.encode(), int(value)))

    def SetDiscreteValue(self, name, value):
        _err(lib().gdgh_unit_set_discrete(self._h, name.encode(), value.encode()))

    def Process(self, x, sample_rate):
        x = _f64(x)
        out = np.empty_like(x)
        lib().gdgh_unit_process(self._h, x.ctypes.data, out.ctypes.data, x.size, sample_rate)
        return out


def delivery_for(session_rate, delivered_rate):
    """The (factor, up, down) of `deliver=` for a (session rate, delivered rate) pair: of the factors 1, 2, 4 that leave an admissible ratio
    (reduced, up <= 160, down <= 320, within a factor of two of 1) the one whose ratio lies closest to 1, so that the long filter at the full
    rate does the most -- (192000, 44100) -> (4, 147, 160), (96000, 44100) -> (2, 147, 160), (88200, 48000) -> (2, 160, 147),
    (192000, 48000) -> (4, 1, 1).  ValueError where no admissible triple exists."""
    from fractions import Fraction
    from math import gcd
    session_rate, delivered_rate = int(session_rate), int(delivered_rate)
    best = None
    if session_rate > 0 and delivered_rate > 0:
        for factor in (1, 2, 4):
            if session_rate % factor:
                continue
            g = gcd(delivered_rate, session_rate // factor)
            up, down = delivered_rate // g, session_rate // factor // g
            if 1 <= up <= 160 and 1 <= down <= 320 and down <= 2 * up and up <= 2 * down:
                away = Fraction(max(up, down), min(up, down))
                if best is None or away < best[0]:
                    best = (away, (factor, up, down))
    if best is None:
        raise ValueError("no delivery factor of 1, 2, 4 with an admissible ratio takes %d Hz to %d Hz" % (session_rate, delivered_rate))
    return best[1]


def filter_compile(taps, sample_rate, compensation_db, order, level_db):
    """Reduce(order) -> Normalize -> Multiply(level) of one IR, as poweramp.compile does per slot."""
    t = _f64(taps)
    cap = max(t.size, order if order else 0) + 8
    out = np.zeros(cap)
    n = lib().gdgh_filter_compile(t.ctypes.data, t.size, sample_rate, compensation_db, order, level_db, out.ctypes.data, cap)
    return out[:n]
