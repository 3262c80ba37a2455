"""
Python face of the batch extension (include/pv_koala_batch.h): B lock-stepped streams on one MI355X.
The reference has no counterpart (one stream per handle, include/pv_koala.h:65-80); stream b of a batch is
sample-for-sample what its own `Koala` instance would produce.
"""

import os
from ctypes import POINTER, Structure, byref, c_char_p, c_double, c_float, c_int32, c_int64, c_uint8, c_uint32, c_void_p, sizeof
from typing import Optional

import numpy as np

from ._koala import (KoalaError, KoalaInvalidArgumentError, KoalaIOError, PicovoiceStatuses, attenuation_limit_to_gain, load_library,
                     raise_status)
from . import bands
from . import level as level_rule
from . import limiter as limiter_rule
from . import comfort as comfort_rule
from .channels import LINK_CHANNELS, MAX_CHANNELS
from .formats import DTYPES, FORMATS
from .packets import FRACTIONAL_UP, inner_samples

PRECISION_FP32 = 0
PRECISION_BF16 = 1
KERNEL_CLASSES = ('analysis', 'gemm_input', 'gru_recurrent', 'gemm_head', 'synthesis')


class BatchCall(Structure):
    """pv_koala_batch_call_t (include/pv_koala_batch.h)"""
    _fields_ = [('struct_size', c_int32), ('num_frames', c_int32), ('pcm', c_void_p), ('enhanced', c_void_p), ('reset', c_void_p),
                ('hold', c_void_p), ('report', c_void_p), ('asynchronous', c_int32)]


class BatchPackets(Structure):
    """pv_koala_batch_packets_t (include/pv_koala_batch.h)"""
    _fields_ = [('struct_size', c_int32), ('max_samples', c_int32), ('counts', c_void_p), ('pcm', c_void_p), ('enhanced', c_void_p),
                ('restart', c_void_p), ('report', c_void_p), ('report_frames', c_int32), ('frames', c_void_p)]


class BatchConfig(Structure):
    """pv_koala_batch_config_t (include/pv_koala_batch.h)"""
    _fields_ = [('struct_size', c_int32), ('num_streams', c_int32), ('max_frames_per_call', c_int32), ('max_samples_per_call', c_int32),
                ('precision', c_int32), ('sample_rate', c_int32), ('sample_format', c_int32)]


class LevelSetting(Structure):
    """pv_koala_level_t (include/pv_koala_batch.h)"""
    _fields_ = [('struct_size', c_int32), ('on', c_int32)] + [(name, c_float) for name in level_rule.FIELDS]

    @classmethod
    def of(cls, setting):
        """a koala_amd.level.Setting, or None (off)"""
        s = level_rule.OFF if setting is None else setting
        if not isinstance(s, level_rule.Setting):
            raise KoalaInvalidArgumentError("a level setting should be a koala_amd.level.Setting (koala_amd.level.settings(...)) or None")
        try:
            level_rule.check(s)
        except (ValueError, TypeError) as e:
            raise KoalaInvalidArgumentError(str(e))
        return cls(sizeof(cls), int(s.on), *[float(v) for v in s[1:]])

    def setting(self):
        return level_rule.Setting(int(self.on), *[float(getattr(self, name)) for name in level_rule.FIELDS])


class LimiterSetting(Structure):
    """pv_koala_limiter_t (include/pv_koala_batch.h)"""
    _fields_ = [('struct_size', c_int32), ('on', c_int32)] + [(name, c_float) for name in limiter_rule.FIELDS]

    @classmethod
    def of(cls, setting):
        """a koala_amd.limiter.Setting, or None (off)"""
        s = limiter_rule.OFF if setting is None else setting
        if not isinstance(s, limiter_rule.Setting):
            raise KoalaInvalidArgumentError("a limiter setting should be a koala_amd.limiter.Setting (koala_amd.limiter.settings(...)) or None")
        try:
            limiter_rule.check(s)
        except (ValueError, TypeError) as e:
            raise KoalaInvalidArgumentError(str(e))
        return cls(sizeof(cls), int(s.on), *[float(v) for v in s[1:]])

    def setting(self):
        return limiter_rule.Setting(int(self.on), *[float(getattr(self, name)) for name in limiter_rule.FIELDS])


class ComfortSetting(Structure):
    """pv_koala_comfort_t (include/pv_koala_batch.h)"""
    _fields_ = [('struct_size', c_int32), ('on', c_int32), ('seed', c_uint32)]


class KoalaBatch(object):
    sample_format, _dtype, _dtype_name = 's16', np.int16, 'int16'  # (what a handle is unless it was made with a sample format)
    channels = 1  # (... or with channels)

    def __init__(self, access_key: str, model_path: str, device: str, library_path: str, num_streams: int,
                 max_frames_per_call: int = 1, precision: str = 'fp32', sample_rate: int = 16000, packet_samples: int = 0, sample_format: str = 's16',
                 channels: int = 1, channel_link: Optional[str] = None, high_band: Optional[str] = None, band_profile=None, level=None, comfort_noise=None, limiter=None) -> None:
        """`sample_rate`: 44100 or 22050 Hz make a packet handle around fractional converters (`packet_samples` > 0 is required; there is
        no frame length, `frame_length` is None, and stream records and the asynchronous calls are refused); otherwise
        8000, 12000, 16000, 24000, 32000 or 48000 Hz, fixed for the handle (include/pv_koala_batch.h, pv_koala_batch_init_rate).  Every
        array of samples is [num_streams, T * frame_length] with frame_length = sample_rate * 256 / 16000; at a rate other than 16000 the
        handle converts on the device, `delay_sample` includes both converters, and the asynchronous calls are refused.
        `packet_samples` > 0 makes a PACKET HANDLE (pv_koala_batch_init_packets): its streams take and deliver any number of samples per call,
        up to `packet_samples`, through `process_packets` / `process_device_packets`; the frame calls are refused on it, `max_frames_per_call`
        is ceil(packet_samples / frame_length) and `delay_sample` grows by frame_length - 1.
        `sample_format`: 's16' (default), 'f32', 'ulaw' or 'alaw' -- what every array of samples that goes in or comes out holds: np.int16,
        np.float32 in [-1, 1) or np.uint8 G.711 bytes (koala_amd.formats has the codecs).  The handle converts on the device around the
        unchanged int16 call (pv_koala_batch_init_config): its result is formats.encode(the 's16' handle(formats.decode(x))), delay, frame
        length and stream records are the 's16' handle's, and the asynchronous calls are refused.  An array of another dtype is refused.
        `channels`: 1 (default) ... 8 -- the memory layout of every array of samples that goes in or comes out of `process`, `process_resets`,
        `process_hold`, `process_call` and `process_packets`: [num_streams / channels, n * channels] (or [.., n, channels], the same memory),
        in which sample i of stream g * channels + c is element [g, i * channels + c] (pv_koala_batch_init_channels; koala_amd.channels has
        the layout in numpy).  The handle splits and joins on the device around the unchanged call: its result is
        channels.interleave(the handle without channels(channels.deinterleave(x))).  Everything per stream -- reset, hold, counts, restart,
        report, gains, records -- stays [num_streams], a packet call's counts must be equal within a group, the device-pointer methods take
        the same layout, and the asynchronous calls are refused.
        `channel_link`: None (default) or 'max' -- with 'max' (`channels` 2, 4 or 8) the channels of a group share one mask, the max of their
        own masks bin by bin, so the stereo image does not move (`set_channel_link`; koala_amd.channels.link_masks states the rule).
        `high_band`: None (default) or 'carry' -- a frame handle at 32000 or 48000 Hz adds the band above the 16 kHz call's, delayed like
        the call and scaled by a broadband gain from the call's masks (`set_high_band`; koala_amd.highband states the rule).
        `band_profile`: None (default) or (floor, ceiling) -- `set_band_profile(floor, ceiling)` on every stream of the new handle.
        `level`: None (default) or a koala_amd.level.Setting -- `set_level(level)` on every stream of the new handle: the output leveller.
        `limiter`: None (default) or a koala_amd.limiter.Setting -- `set_limiter(limiter)` on every stream of the new handle: the peak limiter.
        `comfort_noise`: None (default), an amplitude curve float32 [257] (koala_amd.comfort.curve(-60)) or a pair (curve, seed) --
        `set_comfort_noise` on every stream of the new handle; with a bare curve or seed None stream b gets the seed b."""
        if not isinstance(access_key, str) or len(access_key) == 0:
            raise KoalaInvalidArgumentError("`access_key` should be a non-empty string.")
        if not os.path.exists(model_path):
            raise KoalaIOError("Could not find model file at `%s`." % model_path)
        if precision not in ('fp32', 'bf16'):
            raise KoalaInvalidArgumentError("`precision` should be `fp32` or `bf16`.")
        fractional = sample_rate in FRACTIONAL_UP
        if sample_rate not in (8000, 12000, 16000, 24000, 32000, 48000) and not fractional:
            raise KoalaInvalidArgumentError("`sample_rate` should be 8000, 12000, 16000, 24000, 32000 or 48000 (22050 and 44100: packet handles only).")
        if not isinstance(packet_samples, int) or packet_samples < 0:
            raise KoalaInvalidArgumentError("`packet_samples` should be a positive number of samples (0: a frame handle).")
        if fractional and not packet_samples:
            raise KoalaInvalidArgumentError("`sample_rate` %d needs `packet_samples` > 0: a handle at this rate must be a packet handle." % sample_rate)
        if not isinstance(sample_format, str) or sample_format not in FORMATS:
            raise KoalaInvalidArgumentError("`sample_format` should be `s16`, `f32`, `ulaw` or `alaw`.")
        if isinstance(channels, bool) or not isinstance(channels, int) or not 1 <= channels <= MAX_CHANNELS:
            raise KoalaInvalidArgumentError("`channels` should be an integer in [1, %d]." % MAX_CHANNELS)
        if not isinstance(num_streams, int) or num_streams % channels:
            raise KoalaInvalidArgumentError("`num_streams` %r is not a multiple of `channels` %d: stream g * channels + c is channel c of group g."
                                            % (num_streams, channels))
        self.channels = channels
        link = self._link_value(channel_link)  # (checked before the handle is made)
        carry = self._high_band_value(high_band)
        if level is not None:  # (checked before any library is loaded)
            LevelSetting.of(level)
        if limiter is not None:  # (checked before any library is loaded)
            LimiterSetting.of(limiter)
        if comfort_noise is not None:  # (checked before any library is loaded)
            pair = comfort_noise if isinstance(comfort_noise, tuple) else (comfort_noise, None)
            if len(pair) != 2:
                raise KoalaInvalidArgumentError("`comfort_noise` should be an amplitude curve, a pair (curve, seed) or None.")
            comfort_noise = (self._comfort_curve(pair[0], num_streams), pair[1])
        if band_profile is not None:  # (checked before any library is loaded)
            if not isinstance(band_profile, (tuple, list)) or len(band_profile) != 2:
                raise KoalaInvalidArgumentError("`band_profile` should be a pair (floor, ceiling) or None.")
            band_profile = self._profile_arrays(band_profile[0], band_profile[1], num_streams)
        if carry and (sample_rate not in (32000, 48000) or packet_samples):
            raise KoalaInvalidArgumentError("`high_band` 'carry' needs a frame handle whose `sample_rate` is 32000 or 48000.")
        self.sample_format = sample_format
        self._dtype = DTYPES[sample_format]
        self._dtype_name = np.dtype(self._dtype).name
        lib = load_library(library_path)
        lib.pv_set_sdk(b'python')
        self._lib = lib
        lib.pv_koala_batch_init.argtypes = [c_char_p, c_char_p, c_char_p, c_int32, c_int32, c_int32, POINTER(c_void_p)]
        lib.pv_koala_batch_init.restype = PicovoiceStatuses
        for name, args in (('process_chunk', [c_void_p, c_int32, c_void_p, c_void_p]), ('process_chunk_async', [c_void_p, c_int32, c_void_p, c_void_p]),
                           ('async_wait', [c_void_p, c_int32]), ('reset', [c_void_p, c_void_p]),
                           ('set_stream', [c_void_p, c_void_p]), ('synchronize', [c_void_p]),
                           ('profile_enable', [c_void_p, c_int32]),
                           ('profile_read', [c_void_p, POINTER(c_double), POINTER(c_int64)]),
                           ('delay_sample', [c_void_p, POINTER(c_int32)]),
                           ('process_chunk_resets', [c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
                           ('process_chunk_resets_async', [c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
                           ('state_size', [c_void_p, POINTER(c_int32)]),
                           ('export_state', [c_void_p, c_int32, c_void_p, c_void_p]),
                           ('import_state', [c_void_p, c_int32, c_void_p, c_void_p]),
                           ('process_chunk_hold', [c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
                           ('set_min_gain', [c_void_p, c_int32, c_void_p, c_void_p]),
                           ('get_min_gain', [c_void_p, c_void_p]),
                           ('set_channel_link', [c_void_p, c_int32]),
                           ('get_channel_link', [c_void_p, POINTER(c_int32)]),
                           ('process_call', [c_void_p, POINTER(BatchCall)])):
            fn = getattr(lib, 'pv_koala_batch_' + name)
            fn.argtypes = args
            fn.restype = PicovoiceStatuses
        lib.pv_koala_batch_delete.argtypes = [c_void_p]
        lib.pv_koala_batch_delete.restype = None
        lib.pv_koala_batch_host_alloc.argtypes = [c_int64, POINTER(c_void_p)]
        lib.pv_koala_batch_host_alloc.restype = PicovoiceStatuses
        lib.pv_koala_batch_host_free.argtypes = [c_void_p]
        lib.pv_koala_batch_host_free.restype = None
        self._pinned = []
        lib.pv_koala_batch_debug_read.argtypes = [c_void_p, c_int32, c_void_p, c_int64]
        lib.pv_koala_batch_debug_read.restype = c_int64

        self._handle = c_void_p()
        prec = PRECISION_BF16 if precision == 'bf16' else PRECISION_FP32
        if packet_samples:
            lib.pv_koala_batch_process_packets.argtypes = [c_void_p, POINTER(BatchPackets)]
            lib.pv_koala_batch_process_packets.restype = PicovoiceStatuses
        if sample_format != 's16' or fractional or channels != 1:  # (any other 's16' handle is made as it has always been: init_config would return the same handle)
            lib.pv_koala_batch_init_config.argtypes = [c_char_p, c_char_p, c_char_p, POINTER(BatchConfig), POINTER(c_void_p)]
            lib.pv_koala_batch_init_config.restype = PicovoiceStatuses
            config = BatchConfig(sizeof(BatchConfig), num_streams, max_frames_per_call, packet_samples, prec, sample_rate,
                                 FORMATS.index(sample_format))
            if channels != 1:
                lib.pv_koala_batch_init_channels.argtypes = [c_char_p, c_char_p, c_char_p, POINTER(BatchConfig), c_int32, POINTER(c_void_p)]
                lib.pv_koala_batch_init_channels.restype = PicovoiceStatuses
                status = lib.pv_koala_batch_init_channels(access_key.encode(), model_path.encode(), device.encode(), byref(config), channels,
                                                          byref(self._handle))
            else:
                status = lib.pv_koala_batch_init_config(access_key.encode(), model_path.encode(), device.encode(), byref(config), byref(self._handle))
            if fractional:  # (the inner 16 kHz packet handle's: it takes the most inner samples a call can yield)
                max_frames_per_call = -(-inner_samples(packet_samples, sample_rate) // 256)
            elif packet_samples:
                max_frames_per_call = -(-packet_samples // (sample_rate * 256 // 16000))
        elif packet_samples:
            lib.pv_koala_batch_init_packets.argtypes = [c_char_p, c_char_p, c_char_p, c_int32, c_int32, c_int32, c_int32, POINTER(c_void_p)]
            lib.pv_koala_batch_init_packets.restype = PicovoiceStatuses
            status = lib.pv_koala_batch_init_packets(access_key.encode(), model_path.encode(), device.encode(), num_streams, packet_samples,
                                                     prec, sample_rate, byref(self._handle))
            max_frames_per_call = -(-packet_samples // (sample_rate * 256 // 16000))
        elif sample_rate == 16000:
            status = lib.pv_koala_batch_init(access_key.encode(), model_path.encode(), device.encode(), num_streams, max_frames_per_call,
                                             prec, byref(self._handle))
        else:
            lib.pv_koala_batch_init_rate.argtypes = [c_char_p, c_char_p, c_char_p, c_int32, c_int32, c_int32, c_int32, POINTER(c_void_p)]
            lib.pv_koala_batch_init_rate.restype = PicovoiceStatuses
            status = lib.pv_koala_batch_init_rate(access_key.encode(), model_path.encode(), device.encode(), num_streams,
                                                  max_frames_per_call, prec, sample_rate, byref(self._handle))
        if status is not PicovoiceStatuses.SUCCESS:
            raise_status(lib, status, 'Initialization failed')
        self.num_streams = num_streams
        self.max_frames_per_call = max_frames_per_call
        self.packet_samples = packet_samples
        self.precision = precision
        self.frame_length = lib.pv_koala_frame_length()
        self.sample_rate = lib.pv_sample_rate()
        d = c_int32()
        if fractional:  # no whole frame, no stream records yet: the library refuses both queries
            self.frame_length = None
        if sample_rate != 16000:
            for name in ('sample_rate',) if fractional else ('sample_rate', 'frame_length'):
                fn = getattr(lib, 'pv_koala_batch_' + name)
                fn.argtypes = [c_void_p, POINTER(c_int32)]
                fn.restype = PicovoiceStatuses
                self._check(fn(self._handle, byref(d)), 'Failed to get the ' + name)
                setattr(self, name, d.value)
        self._check(lib.pv_koala_batch_delay_sample(self._handle, byref(d)), 'Failed to get delay samples')
        self.delay_sample = d.value
        self.state_size = 0  # bytes of one stream record (export_state / import_state)
        if not fractional:
            self._check(lib.pv_koala_batch_state_size(self._handle, byref(d)), 'Failed to get the state size')
            self.state_size = d.value
        if link or carry or band_profile is not None or level is not None or comfort_noise is not None or limiter is not None:
            try:
                if comfort_noise is not None:
                    self.set_comfort_noise(comfort_noise[0], comfort_noise[1])
                if level is not None:
                    self.set_level(level)
                if limiter is not None:
                    self.set_limiter(limiter)
                if band_profile is not None:
                    self.set_band_profile(band_profile[0], band_profile[1])
                if link:
                    self.set_channel_link(channel_link)
                if carry:
                    self.set_high_band(high_band)
            except Exception:
                self.delete()
                raise

    @staticmethod
    def _high_band_value(mode):
        if mode is not None and mode != 'carry':
            raise KoalaInvalidArgumentError("`high_band` should be 'carry' or None.")
        return 1 if mode else 0

    def _high_band_fn(self, which, arg):
        # (bound at first use, not with the others in __init__: developer A/B runs load libraries built before the entry points existed)
        fn = getattr(self._lib, 'pv_koala_batch_%s_high_band' % which)
        fn.argtypes, fn.restype = [c_void_p, arg], PicovoiceStatuses
        return fn

    def set_high_band(self, mode: Optional[str]) -> None:
        """'carry': from the next call on, the handle (a frame handle at 32000 or 48000 Hz) adds the band the 16 kHz call never saw to its
        output, delayed by `delay_sample` and scaled by a smooth broadband gain from the call's own masks (include/pv_koala_batch.h,
        pv_koala_batch_set_high_band; koala_amd.highband states the rule).  The high band is that of streams that begin with that call.
        None: exactly the handle it was.  While it is on, `hold`, per-frame resets behind frame 0 and stream records are refused."""
        self._check(self._high_band_fn('set', c_int32)(self._handle, self._high_band_value(mode)), 'set_high_band failed')

    @property
    def high_band(self) -> Optional[str]:
        v = c_int32()
        self._check(self._high_band_fn('get', POINTER(c_int32))(self._handle, byref(v)), 'high_band failed')
        return 'carry' if v.value else None

    def _link_value(self, link):
        if link is not None and link != 'max':
            raise KoalaInvalidArgumentError("`channel_link` should be 'max' or None.")
        if link and self.channels not in LINK_CHANNELS:
            raise KoalaInvalidArgumentError("`channel_link` 'max' needs a handle whose `channels` is 2, 4 or 8: this handle's `channels` is %d."
                                            % self.channels)
        return 1 if link else 0

    def set_channel_link(self, link: Optional[str]) -> None:
        """'max': from the next call on, the mask applied to every stream of a group is the max of the group's masks, bin by bin
        (include/pv_koala_batch.h, pv_koala_batch_set_channel_link; `channels` must be 2, 4 or 8).  None: the channels are independent
        again -- exactly the handle it was.  Configuration, not state: the streams evolve the same either way, only the samples differ.
        A linked call refuses `hold` (and a packet call `restart`, or a phase) that differs within a group."""
        self._check(self._lib.pv_koala_batch_set_channel_link(self._handle, self._link_value(link)), 'set_channel_link failed')

    @property
    def channel_link(self) -> Optional[str]:
        v = c_int32()
        self._check(self._lib.pv_koala_batch_get_channel_link(self._handle, byref(v)), 'channel_link failed')
        return 'max' if v.value else None

    def _check(self, status, what):
        if status is not PicovoiceStatuses.SUCCESS:
            raise_status(self._lib, status, what)

    def _samples(self, pcm):
        """the caller's samples as a C-contiguous array of the handle's dtype; on a handle with a format a wrong dtype is refused, not converted"""
        if self.sample_format != 's16' and (not isinstance(pcm, np.ndarray) or pcm.dtype != self._dtype):
            raise KoalaInvalidArgumentError("expected a %s array: the handle's sample format is `%s`" % (self._dtype_name, self.sample_format))
        return np.ascontiguousarray(pcm, dtype=self._dtype)

    def _rows(self, pcm):
        """(the caller's samples as [num_streams, n] rows of memory, the caller's shape).  On a handle with channels the array is
        [G, n * C] or [G, n, C] and the rows are that memory cut into num_streams equal parts -- the library reads it interleaved --
        so the checks and sizes of every method are those of the handle without channels."""
        a = self._samples(pcm)
        if self.channels == 1:
            return a, a.shape
        C, G = self.channels, self.num_streams // self.channels
        if not ((a.ndim == 2 and a.shape[0] == G and a.shape[1] % C == 0) or (a.ndim == 3 and a.shape[0] == G and a.shape[2] == C)):
            raise KoalaInvalidArgumentError("expected %s array of shape [%d, n*%d] or [%d, n, %d]: the handle's `channels` is %d"
                                            % (self._dtype_name, G, C, G, C, C))
        return a.reshape(self.num_streams, -1), a.shape

    def process(self, pcm: np.ndarray) -> np.ndarray:
        """pcm: int16 [num_streams, T*frame_length] in host memory -> enhanced, same shape (synchronous)."""
        a, shape = self._rows(pcm)
        if a.ndim != 2 or a.shape[0] != self.num_streams or a.shape[1] % self.frame_length:
            raise KoalaInvalidArgumentError("expected %s array of shape [%d, T*%d]" % (self._dtype_name, self.num_streams, self.frame_length))
        out = np.empty_like(a)
        self._check(self._lib.pv_koala_batch_process_chunk(self._handle, a.shape[1] // self.frame_length,
                                                           a.ctypes.data, out.ctypes.data), 'Processing failed')
        return out.reshape(shape)

    def alloc_host(self, num_frames: int) -> np.ndarray:
        """[num_streams, num_frames*frame_length] of the handle's dtype (int16 unless it has a sample format) in page-locked host memory (freed by `delete()`): `process()` on such arrays
        lets the GPU's copy engines move the audio directly instead of through a staging copy."""
        n = self.num_streams * num_frames * self.frame_length
        p = c_void_p()
        nbytes = n * np.dtype(self._dtype).itemsize
        self._check(self._lib.pv_koala_batch_host_alloc(nbytes, byref(p)), 'Host allocation failed')
        self._pinned.append(p)
        buf = (c_uint8 * nbytes).from_address(p.value)
        return np.frombuffer(buf, dtype=self._dtype).reshape(self.num_streams, num_frames * self.frame_length)

    def process_into(self, pcm: np.ndarray, enhanced: np.ndarray) -> None:
        """Like `process()`, writing into a caller-provided array (both C-contiguous int16 of the same shape)."""
        for a in (pcm, enhanced):
            if (not isinstance(a, np.ndarray) or a.dtype != self._dtype or not a.flags['C_CONTIGUOUS'] or a.ndim != 2 or
                    a.shape[0] != self.num_streams or a.shape[1] % self.frame_length or a.shape != pcm.shape):
                raise KoalaInvalidArgumentError(
                    "expected C-contiguous %s arrays of shape [%d, T*%d]" % (self._dtype_name, self.num_streams, self.frame_length))
        self._check(self._lib.pv_koala_batch_process_chunk(self._handle, pcm.shape[1] // self.frame_length,
                                                           pcm.ctypes.data, enhanced.ctypes.data), 'Processing failed')

    def process_async(self, pcm: np.ndarray, enhanced: np.ndarray) -> None:
        """`process_into()` without the wait, for page-locked arrays (`alloc_host()`): the call is enqueued and returns; up to three are
        in flight, so a caller that rotates over three buffer pairs keeps the link and the GPU busy at once.  `enhanced` is valid
        after `synchronize()` or once `wait(k)` says the call is no longer among the k in flight."""
        for a in (pcm, enhanced):
            if (not isinstance(a, np.ndarray) or a.dtype != self._dtype or not a.flags['C_CONTIGUOUS'] or a.ndim != 2 or
                    a.shape[0] != self.num_streams or a.shape[1] % self.frame_length or a.shape != pcm.shape):
                raise KoalaInvalidArgumentError(
                    "expected C-contiguous %s arrays of shape [%d, T*%d]" % (self._dtype_name, self.num_streams, self.frame_length))
        self._check(self._lib.pv_koala_batch_process_chunk_async(self._handle, pcm.shape[1] // self.frame_length,
                                                                 pcm.ctypes.data, enhanced.ctypes.data), 'Processing failed')

    def wait(self, max_in_flight: int = 0) -> None:
        """Blocks until at most `max_in_flight` asynchronous calls are still in flight (0: all done).  Triple buffering: before reusing
        buffer pair n % 3 for call n, `wait(2)` -- call n - 3 has completed, its output may be taken and its input refilled."""
        self._check(self._lib.pv_koala_batch_async_wait(self._handle, max_in_flight), 'wait failed')

    def process_device(self, num_frames: int, pcm_ptr: int, enhanced_ptr: int) -> None:
        """Device pointers (e.g. torch_tensor.data_ptr()) of int16 [num_streams, num_frames*frame_length]; asynchronous."""
        self._check(self._lib.pv_koala_batch_process_chunk(self._handle, num_frames, c_void_p(pcm_ptr),
                                                           c_void_p(enhanced_ptr)), 'Processing failed')

    def _reset_mask(self, reset, num_frames):
        """(mask array kept alive by the caller's frame, pointer) for a per-frame reset mask [num_streams, num_frames], or (None, None)"""
        if reset is None:
            return None, None
        m = np.ascontiguousarray(reset, dtype=np.uint8)
        if m.shape != (self.num_streams, num_frames):
            raise KoalaInvalidArgumentError("`reset` must have shape [%d, %d]" % (self.num_streams, num_frames))
        return m, m.ctypes.data

    def process_resets(self, pcm: np.ndarray, reset: Optional[np.ndarray]) -> np.ndarray:
        """`process()` with per-frame stream resets: reset[b, t] != 0 restarts stream b from the fresh state right before frame t of this
        call (include/pv_koala_batch.h, pv_koala_batch_process_chunk_resets).  `reset`: [num_streams, T] (None: no resets)."""
        a, shape = self._rows(pcm)
        if a.ndim != 2 or a.shape[0] != self.num_streams or a.shape[1] % self.frame_length:
            raise KoalaInvalidArgumentError("expected %s array of shape [%d, T*%d]" % (self._dtype_name, self.num_streams, self.frame_length))
        T = a.shape[1] // self.frame_length
        m, mp = self._reset_mask(reset, T)
        out = np.empty_like(a)
        self._check(self._lib.pv_koala_batch_process_chunk_resets(self._handle, T, a.ctypes.data, out.ctypes.data, mp),
                    'Processing failed')
        return out.reshape(shape)

    def process_async_resets(self, pcm: np.ndarray, enhanced: np.ndarray, reset: Optional[np.ndarray]) -> None:
        """`process_async()` with per-frame stream resets ([num_streams, T]); the mask is copied before the call returns."""
        for a in (pcm, enhanced):
            if (not isinstance(a, np.ndarray) or a.dtype != self._dtype or not a.flags['C_CONTIGUOUS'] or a.ndim != 2 or
                    a.shape[0] != self.num_streams or a.shape[1] % self.frame_length or a.shape != pcm.shape):
                raise KoalaInvalidArgumentError(
                    "expected C-contiguous %s arrays of shape [%d, T*%d]" % (self._dtype_name, self.num_streams, self.frame_length))
        T = pcm.shape[1] // self.frame_length
        m, mp = self._reset_mask(reset, T)
        self._check(self._lib.pv_koala_batch_process_chunk_resets_async(self._handle, T, pcm.ctypes.data, enhanced.ctypes.data, mp),
                    'Processing failed')

    def process_device_resets(self, num_frames: int, pcm_ptr: int, enhanced_ptr: int, reset: Optional[np.ndarray]) -> None:
        """`process_device()` with per-frame stream resets: the host mask [num_streams, num_frames] is read before the call returns, the
        work is enqueued on the handle's stream."""
        m, mp = self._reset_mask(reset, num_frames)
        self._check(self._lib.pv_koala_batch_process_chunk_resets(self._handle, num_frames, c_void_p(pcm_ptr), c_void_p(enhanced_ptr), mp),
                    'Processing failed')

    # ---- one call with everything it may carry, the frame report included (include/pv_koala_batch.h, pv_koala_batch_process_call)

    def _call(self, num_frames, pcm_ptr, enhanced_ptr, reset, hold, report_ptr, asynchronous):
        m, mp = self._reset_mask(reset, num_frames)
        h, hp = self._hold_mask(hold)
        call = BatchCall(sizeof(BatchCall), num_frames, pcm_ptr, enhanced_ptr, mp, hp, report_ptr or None, 1 if asynchronous else 0)
        self._check(self._lib.pv_koala_batch_process_call(self._handle, byref(call)), 'Processing failed')

    def _audio(self, *arrays):
        for a in arrays:
            if (not isinstance(a, np.ndarray) or a.dtype != self._dtype or not a.flags['C_CONTIGUOUS'] or a.ndim != 2 or
                    a.shape[0] != self.num_streams or a.shape[1] == 0 or a.shape[1] % self.frame_length or a.shape != arrays[0].shape):
                raise KoalaInvalidArgumentError(
                    "expected C-contiguous %s arrays of shape [%d, T*%d]" % (self._dtype_name, self.num_streams, self.frame_length))
        return arrays[0].shape[1] // self.frame_length

    def _report_array(self, report, num_frames):
        if (not isinstance(report, np.ndarray) or report.dtype != np.float32 or not report.flags['C_CONTIGUOUS'] or
                report.shape != (self.num_streams, num_frames, 4)):
            raise KoalaInvalidArgumentError("`report` must be a C-contiguous float32 array of shape [%d, %d, 4]" % (self.num_streams, num_frames))
        return report.ctypes.data

    def process_call(self, pcm: np.ndarray, reset: Optional[np.ndarray] = None, hold: Optional[np.ndarray] = None, report: bool = False):
        """`process()` with any of: per-frame resets ([num_streams, T]), held streams ([num_streams]; not together with resets), and the
        FRAME REPORT.  Returns `enhanced`, or `(enhanced, report)` when `report` is true: float32 [num_streams, T, 4] = e_in, e_out,
        mask_sum, 0 of every stream and frame (include/pv_koala_batch.h; koala_amd.report turns rows into dBFS, dB of suppression and
        mean gain).  The samples do not depend on whether the report is asked for."""
        a, shape = self._rows(pcm)
        T = self._audio(a)
        out = np.empty_like(a)
        rep = np.empty((self.num_streams, T, 4), np.float32) if report else None
        self._call(T, a.ctypes.data, out.ctypes.data, reset, hold, rep.ctypes.data if report else None, False)
        return (out.reshape(shape), rep) if report else out.reshape(shape)

    def process_device_call(self, num_frames: int, pcm_ptr: int, enhanced_ptr: int, report_ptr: int = 0, reset: Optional[np.ndarray] = None,
                            hold: Optional[np.ndarray] = None) -> None:
        """`process_device()` with any of resets, held streams (host masks, read before the call returns) and the frame report:
        `report_ptr` is a device pointer of float32 [num_streams, num_frames, 4] (0: none), written on the handle's stream."""
        self._call(num_frames, c_void_p(pcm_ptr), c_void_p(enhanced_ptr), reset, hold, c_void_p(report_ptr) if report_ptr else None, False)

    def alloc_host_report(self, num_frames: int) -> np.ndarray:
        """float32 [num_streams, num_frames, 4] in page-locked host memory (freed by `delete()`): the report array of `process_async_call`."""
        n = self.num_streams * num_frames * 4
        p = c_void_p()
        self._check(self._lib.pv_koala_batch_host_alloc(4 * n, byref(p)), 'Host allocation failed')
        self._pinned.append(p)
        return np.frombuffer((c_float * n).from_address(p.value), dtype=np.float32).reshape(self.num_streams, num_frames, 4)

    def process_async_call(self, pcm: np.ndarray, enhanced: np.ndarray, report: Optional[np.ndarray] = None,
                           reset: Optional[np.ndarray] = None) -> None:
        """`process_async()` with per-frame resets and / or the frame report: `report` is a page-locked float32 [num_streams, T, 4]
        (`alloc_host_report()`), valid when `enhanced` is -- after `synchronize()` or once `wait(k)` says the call has completed."""
        T = self._audio(pcm, enhanced)
        rp = None if report is None else self._report_array(report, T)
        self._call(T, pcm.ctypes.data, enhanced.ctypes.data, reset, None, rp, True)

    def _stream_list(self, streams, n):
        """(int32 array kept alive by the caller's frame, pointer, count) for a list of stream indices (None: 0 .. n - 1)"""
        if streams is None:
            return None, None, self.num_streams if n is None else n
        s = np.ascontiguousarray(streams)
        if s.ndim != 1 or s.size == 0 or not np.issubdtype(s.dtype, np.integer):
            raise KoalaInvalidArgumentError("`streams` must be a non-empty list of stream indices")
        if n is not None and s.size != n:
            raise KoalaInvalidArgumentError("`streams` has %d entries for %d records" % (s.size, n))
        s = s.astype(np.int32)
        return s, s.ctypes.data, int(s.size)

    def export_state(self, streams=None) -> np.ndarray:
        """The state of the listed streams (None: all) as records: uint8 [n, state_size], record i = stream streams[i].  A record is
        plain bytes (include/pv_koala_batch.h): `bytes(blob[i])` can go to a database and come back in another process, into any
        slot of any handle on the same model and precision."""
        s, sp, n = self._stream_list(streams, None)
        out = np.empty((n, self.state_size), np.uint8)
        self._check(self._lib.pv_koala_batch_export_state(self._handle, n, sp, out.ctypes.data), 'export_state failed')
        return out

    def import_state(self, blobs, streams=None) -> None:
        """Continues the listed streams (None: slots 0 .. n - 1) from records: `blobs` is uint8 [n, state_size], a list of n `bytes`
        objects of state_size each, or one such object."""
        if isinstance(blobs, (bytes, bytearray, memoryview)):
            blobs = [blobs]
        if isinstance(blobs, (list, tuple)):
            if any(not isinstance(b, (bytes, bytearray, memoryview, np.ndarray)) or len(b) != self.state_size for b in blobs):
                raise KoalaInvalidArgumentError("every record must be %d bytes" % self.state_size)
            blobs = np.frombuffer(b''.join(bytes(b) for b in blobs), np.uint8).reshape(len(blobs), self.state_size)
        a = np.ascontiguousarray(blobs)
        if a.dtype != np.uint8 or a.ndim != 2 or a.shape[1] != self.state_size:
            raise KoalaInvalidArgumentError("expected uint8 records of shape [n, %d]" % self.state_size)
        s, sp, n = self._stream_list(streams, a.shape[0])
        self._check(self._lib.pv_koala_batch_import_state(self._handle, n, sp, a.ctypes.data), 'import_state failed')

    def _hold_mask(self, hold):
        if hold is None:
            return None, None
        m = np.ascontiguousarray(hold, dtype=np.uint8)
        if m.shape != (self.num_streams,):
            raise KoalaInvalidArgumentError("`hold` must have one entry per stream")
        return m, m.ctypes.data

    def process_hold(self, pcm: np.ndarray, hold: Optional[np.ndarray]) -> np.ndarray:
        """`process()` in which the streams with hold[b] != 0 are not advanced (their state stays bit for bit what it was; their rows of
        the result are unspecified).  `hold`: [num_streams] (None: nobody)."""
        a, shape = self._rows(pcm)
        if a.ndim != 2 or a.shape[0] != self.num_streams or a.shape[1] % self.frame_length:
            raise KoalaInvalidArgumentError("expected %s array of shape [%d, T*%d]" % (self._dtype_name, self.num_streams, self.frame_length))
        m, mp = self._hold_mask(hold)
        out = np.empty_like(a)
        self._check(self._lib.pv_koala_batch_process_chunk_hold(self._handle, a.shape[1] // self.frame_length, a.ctypes.data,
                                                                out.ctypes.data, mp), 'Processing failed')
        return out.reshape(shape)

    def process_device_hold(self, num_frames: int, pcm_ptr: int, enhanced_ptr: int, hold: Optional[np.ndarray]) -> None:
        """`process_device()` with held streams: the host mask [num_streams] is read before the call returns, the work is enqueued on
        the handle's stream."""
        m, mp = self._hold_mask(hold)
        self._check(self._lib.pv_koala_batch_process_chunk_hold(self._handle, num_frames, c_void_p(pcm_ptr), c_void_p(enhanced_ptr), mp),
                    'Processing failed')

    # ---- packet handles (include/pv_koala_batch.h, pv_koala_batch_process_packets)

    def _packets(self, max_samples, counts, pcm_ptr, enhanced_ptr, restart, report_ptr, report_frames):
        if not self.packet_samples:
            raise KoalaInvalidArgumentError("not a packet handle: create it with `packet_samples`")
        n = np.ascontiguousarray(counts, dtype=np.int32)
        if n.shape != (self.num_streams,):
            raise KoalaInvalidArgumentError("`counts` must have one entry per stream")
        r, rp = self._hold_mask(restart) if restart is not None else (None, None)
        frames = np.zeros(self.num_streams, np.int32)
        call = BatchPackets(sizeof(BatchPackets), max_samples, n.ctypes.data, pcm_ptr, enhanced_ptr, rp, report_ptr or None, report_frames,
                            frames.ctypes.data)
        self._check(self._lib.pv_koala_batch_process_packets(self._handle, byref(call)), 'Processing failed')
        return frames

    def process_packets(self, pcm: np.ndarray, counts, restart=None, report: bool = False):
        """One call of a packet handle.  pcm: int16 [num_streams, max_samples] in host memory, of which row b's first counts[b] samples
        count (0: the stream is stalled and not advanced); `restart`: [num_streams] or None, non-zero = the stream is fresh before this
        packet.  Returns `enhanced` (same shape; row b's first counts[b] samples are the stream's next output samples, the rest zeros),
        or `(enhanced, frames, report)` when `report` is true: frames int32 [num_streams] = the frames each stream completed in the call,
        report float32 [num_streams, max(frames), 4] with stream b's rows [0, frames[b]) filled."""
        a, shape = self._rows(pcm)
        if a.ndim != 2 or a.shape[0] != self.num_streams or a.shape[1] < 1:
            raise KoalaInvalidArgumentError("expected %s array of shape [%d, max_samples]" % (self._dtype_name, self.num_streams))
        out = np.zeros_like(a)
        if not report:
            self._packets(a.shape[1], counts, a.ctypes.data, out.ctypes.data, restart, None, 0)
            return out.reshape(shape)
        # (a stream completes at most this many frames; at 44 100 / 22 050 Hz the rows are the inner 16 kHz stream's)
        rows = a.shape[1] // self.frame_length + 1 if self.frame_length else inner_samples(a.shape[1], self.sample_rate) // 256 + 1
        rep = np.zeros((self.num_streams, rows, 4), np.float32)
        frames = self._packets(a.shape[1], counts, a.ctypes.data, out.ctypes.data, restart, rep.ctypes.data, rows)
        return out.reshape(shape), frames, rep[:, :int(frames.max()) if frames.size else 0]

    def process_device_packets(self, max_samples: int, counts, pcm_ptr: int, enhanced_ptr: int, restart=None, report_ptr: int = 0,
                               report_frames: int = 0) -> np.ndarray:
        """`process_packets` for device pointers of int16 [num_streams, max_samples] (and float32 [num_streams, report_frames, 4]):
        `counts` and `restart` are host arrays read before the call returns, the work is enqueued on the handle's stream without a host
        wait.  Returns frames int32 [num_streams]."""
        return self._packets(max_samples, counts, c_void_p(pcm_ptr), c_void_p(enhanced_ptr), restart,
                             c_void_p(report_ptr) if report_ptr else None, report_frames)

    def set_min_gain(self, gains, streams=None) -> None:
        """Per-stream attenuation limit as a minimum mask gain in [0, 1] (include/pv_koala_batch.h, pv_koala_batch_set_min_gain): 0 = no
        limit, 1 = bypass with unchanged latency, in between no bin of the stream is attenuated by more than -20 log10(gain) dB.
        `gains`: one value per listed stream, or a scalar for all of them; `streams`: indices (None: every stream, in order).  Holds from
        the next call on; configuration, not state: resets, held streams and stream records neither change nor carry it."""
        g = np.asarray(gains, dtype=np.float32)
        if g.ndim == 0:
            g = np.full(self.num_streams if streams is None else np.size(streams), g, np.float32)
        g = np.ascontiguousarray(g)
        if g.ndim != 1 or g.size == 0 or (streams is None and g.size != self.num_streams):
            raise KoalaInvalidArgumentError("`gains` must be a scalar or one value per listed stream")
        s, sp, n = self._stream_list(streams, g.size)
        self._check(self._lib.pv_koala_batch_set_min_gain(self._handle, n, sp, g.ctypes.data), 'set_min_gain failed')

    def set_attenuation_limit(self, db, streams=None) -> None:
        """`set_min_gain` in dB: the listed streams are suppressed by at most `db` dB (scalar or one value per stream; None or inf:
        unlimited; 0: bypass).  Negative or NaN limits raise ValueError."""
        self.set_min_gain(attenuation_limit_to_gain(db), streams)

    def min_gain(self) -> np.ndarray:
        """The minimum gains in force, float32 [num_streams]."""
        out = np.empty(self.num_streams, np.float32)
        self._check(self._lib.pv_koala_batch_get_min_gain(self._handle, out.ctypes.data), 'min_gain failed')
        return out

    @staticmethod
    def _profile_arrays(floor, ceiling, rows):
        try:
            return bands.check(floor, ceiling, rows)
        except ValueError as e:
            raise KoalaInvalidArgumentError(str(e))

    def _band_profile_fn(self, which, args):
        # (bound at first use, like the high band's: developer A/B runs load libraries built before the entry points existed)
        fn = getattr(self._lib, 'pv_koala_batch_%s_band_profile' % which)
        fn.argtypes, fn.restype = args, PicovoiceStatuses
        return fn

    def set_band_profile(self, floor=None, ceiling=None, streams=None) -> None:
        """Per-stream, per-bin floor and ceiling on the mask (include/pv_koala_batch.h, pv_koala_batch_set_band_profile): in every bin k
        the mask m' under the attenuation limit becomes min(ceiling[k], max(floor[k], m')).  `floor`, `ceiling`: float32 [257] for all
        the listed streams or [n, 257], one row per listed stream, values in [0, 1], floor <= ceiling; None: zeros / ones, so
        `set_band_profile()` restores the neutral profile.  `streams`: indices (None: every stream, in order).  koala_amd.bands builds
        curves (highpass, bandpass, depth_limit_db) and states the rule.  Holds from the next call on; configuration, not state.  A call
        under a profile that is not neutral is refused while the channel link or the high-band carry is on."""
        s, sp, n = self._stream_list(streams, None)
        lo, hi = self._profile_arrays(floor, ceiling, n)
        fn = self._band_profile_fn('set', [c_void_p, c_int32, c_void_p, c_void_p, c_void_p])
        self._check(fn(self._handle, n, sp, lo.ctypes.data, hi.ctypes.data), 'set_band_profile failed')

    def band_profile(self, stream: int):
        """(floor, ceiling) in force of one stream, float32 [257] each."""
        lo, hi = np.empty(bands.NUM_BINS, np.float32), np.empty(bands.NUM_BINS, np.float32)
        fn = self._band_profile_fn('get', [c_void_p, c_int32, c_void_p, c_void_p])
        self._check(fn(self._handle, int(stream), lo.ctypes.data, hi.ctypes.data), 'band_profile failed')
        return lo, hi

    # ---- output leveller (include/pv_koala_batch.h, OUTPUT LEVELLER; koala_amd.level states the rule)

    def _level_fn(self, name, args):
        # (bound at first use, like the band profile's: developer A/B runs load libraries built before the entry points existed)
        fn = getattr(self._lib, 'pv_koala_batch_' + name)
        fn.argtypes, fn.restype = args, PicovoiceStatuses
        return fn

    # the leveller's, the limiter's and the comfort noise's entry points are one ctypes call each: a table of settings for a stream list,
    # one setting back, the state of a stream list out and in

    def _set_stage(self, name, struct, rule, setting, streams):
        s, sp, n = self._stream_list(streams, None)
        each = list(setting) if isinstance(setting, (list, tuple)) and not isinstance(setting, rule.Setting) else [setting] * n
        if len(each) != n:
            raise KoalaInvalidArgumentError("`setting` must be one setting or one per listed stream")
        table = (struct * n)(*[struct.of(v) for v in each])
        self._check(self._level_fn('set_' + name, [c_void_p, c_int32, c_void_p, c_void_p])(self._handle, n, sp, byref(table)), 'set_%s failed' % name)

    def _get_stage(self, name, struct, stream):
        out = struct(sizeof(struct))
        self._check(self._level_fn('get_' + name, [c_void_p, c_int32, c_void_p])(self._handle, int(stream), byref(out)), name + ' failed')
        return out.setting()

    def _stage_state(self, name, shape, dtype, streams):
        s, sp, n = self._stream_list(streams, None)
        out = np.empty((n,) + shape, dtype)
        self._check(self._level_fn('get_%s_state' % name, [c_void_p, c_int32, c_void_p, c_void_p])(self._handle, n, sp, out.ctypes.data), name + '_state failed')
        return out

    def _set_stage_state(self, name, shape, dtype, what, state, streams):
        a = np.ascontiguousarray(state, dtype=dtype)
        if a.shape[1:] != shape or a.ndim != 1 + len(shape) or a.shape[0] == 0:
            raise KoalaInvalidArgumentError("expected %s of shape [n%s]" % (what, ''.join(', %d' % d for d in shape)))
        s, sp, n = self._stream_list(streams, a.shape[0])
        self._check(self._level_fn('set_%s_state' % name, [c_void_p, c_int32, c_void_p, c_void_p])(self._handle, n, sp, a.ctypes.data), 'set_%s_state failed' % name)

    def set_level(self, setting, streams=None) -> None:
        """The output leveller of the listed streams (None: every stream): `setting` is a koala_amd.level.Setting
        (koala_amd.level.settings(target_dbfs=-23, ...)), None for off, or a list with one of either per listed stream.  While a stream's
        leveller is on, its samples are brought towards the target by a gain that adapts on speech frames only and ramps over every
        frame; what keeps the product under a ceiling is the peak limiter (`set_limiter`), without it saturation alone.  Holds from the next call on; configuration, not state: resets, held streams and stream
        records neither change nor carry it.  A call is refused while some stream levels and the channel link or the high-band carry is
        on, on the asynchronous entry points and at 44100 / 22050 Hz."""
        self._set_stage('level', LevelSetting, level_rule, setting, streams)

    def level(self, stream: int):
        """The koala_amd.level.Setting in force of one stream."""
        return self._get_stage('level', LevelSetting, stream)

    def level_state(self, streams=None) -> np.ndarray:
        """The leveller's state of the listed streams (None: all), float32 [n, 2] = lvl (the tracked speech energy), gain, behind
        everything enqueued on the handle.  Stream records do not carry it: a caller that moves a stream moves these eight bytes too."""
        return self._stage_state('level', (2,), np.float32, streams)

    def set_level_state(self, state, streams=None) -> None:
        """Continues the leveller of the listed streams (None: slots 0 .. n - 1) from `state`, float32 [n, 2] = lvl, gain; (0, 1) is fresh."""
        self._set_stage_state('level', (2,), np.float32, 'float32 state', state, streams)

    # ---- peak limiter (include/pv_koala_batch.h, PEAK LIMITER; koala_amd.limiter states the rule)

    def set_limiter(self, setting, streams=None) -> None:
        """The peak limiter of the listed streams (None: every stream): `setting` is a koala_amd.limiter.Setting
        (koala_amd.limiter.settings(ceiling_dbfs=-1, release_ms=50)), None for off, or a list with one of either per listed stream.  While
        a stream's limiter is on, no sample of its inner 16 kHz output is above the ceiling: the gain falls at once and recovers linearly,
        behind the leveller's ramp and in front of its saturation.  Holds from the next call on; configuration, not state.  A call is
        refused while some stream limits and the channel link or the high-band carry is on, on the asynchronous entry points and at
        44100 / 22050 Hz."""
        self._set_stage('limiter', LimiterSetting, limiter_rule, setting, streams)

    def limiter(self, stream: int):
        """The koala_amd.limiter.Setting in force of one stream."""
        return self._get_stage('limiter', LimiterSetting, stream)

    def limiter_state(self, streams=None) -> np.ndarray:
        """The limiter's state of the listed streams (None: all), float32 [n] = g, the gain behind each stream's last sample, behind
        everything enqueued on the handle.  Stream records do not carry it: a caller that moves a stream moves these four bytes too."""
        return self._stage_state('limiter', (), np.float32, streams)

    def set_limiter_state(self, state, streams=None) -> None:
        """Continues the limiter of the listed streams (None: slots 0 .. n - 1) from `state`, float32 [n] = g in (0, 1]; 1 is fresh."""
        self._set_stage_state('limiter', (), np.float32, 'float32 state', state, streams)

    # ---- comfort noise (include/pv_koala_batch.h, COMFORT NOISE; koala_amd.comfort states the rule)

    @staticmethod
    def _comfort_curve(amplitude, rows):
        try:
            return comfort_rule.check(amplitude, rows)
        except (ValueError, TypeError) as e:
            raise KoalaInvalidArgumentError(str(e))

    def set_comfort_noise(self, amplitude=None, seed=None, streams=None, on=True) -> None:
        """Comfort noise of the listed streams (None: every stream): a low, stationary, shaped noise exactly where the mask removed energy.
        `amplitude`: float32 [257] for all the listed streams or [n, 257], one row per listed stream, finite and >= 0, in the spectrum's
        units (koala_amd.comfort.curve(dbfs, shape) builds one); None: the streams keep their curves.  `seed`: one uint32 for all, one per
        listed stream, or None: a stream keeps the seed it was given before, and one that never got a seed takes its index.  `on=False` (or `set_comfort_noise(on=False)`) switches the streams off and
        keeps curve and seed.  Holds from the next call on; configuration, not state: resets, held streams and stream records neither
        change nor carry it, and the frame counter travels through `comfort_state` / `set_comfort_state`.  A call is refused while some
        stream's comfort noise is on and the channel link or the high-band carry is on, on the asynchronous entry points and at
        44100 / 22050 Hz."""
        s, sp, n = self._stream_list(streams, None)
        amp = None if amplitude is None else self._comfort_curve(amplitude, n)
        idx = np.arange(n) if s is None else np.asarray(s)
        seeded = self.__dict__.setdefault('_comfort_seeded', set())  # (the streams whose seed is the caller's or an index handed out before)
        if seed is None:
            seeds = [self.comfort_noise(int(b))[1] if int(b) in seeded else int(b) for b in idx]
        else:
            seeds = np.broadcast_to(np.asarray(seed), (n,)) if np.ndim(seed) == 0 else np.asarray(seed)
        if len(seeds) != n:
            raise KoalaInvalidArgumentError("`seed` must be one seed or one per listed stream")
        table = (ComfortSetting * n)(*[ComfortSetting(sizeof(ComfortSetting), 1 if on else 0, int(v) & 0xFFFFFFFF) for v in seeds])
        fn = self._level_fn('set_comfort_noise', [c_void_p, c_int32, c_void_p, c_void_p, c_void_p])
        self._check(fn(self._handle, n, sp, byref(table), None if amp is None else amp.ctypes.data), 'set_comfort_noise failed')
        seeded.update(int(b) for b in idx)

    def comfort_noise(self, stream: int):
        """(on, seed, amplitude float32 [257]) in force of one stream."""
        out, amp = ComfortSetting(sizeof(ComfortSetting)), np.empty(comfort_rule.NUM_BINS, np.float32)
        fn = self._level_fn('get_comfort_noise', [c_void_p, c_int32, c_void_p, c_void_p])
        self._check(fn(self._handle, int(stream), byref(out), amp.ctypes.data), 'comfort_noise failed')
        return bool(out.on), int(out.seed), amp

    def comfort_state(self, streams=None) -> np.ndarray:
        """The frame counters of the listed streams (None: all), uint32 [n], behind everything enqueued on the handle.  Stream records do
        not carry them: a caller that moves a stream moves these four bytes too."""
        return self._stage_state('comfort', (), np.uint32, streams)

    def set_comfort_state(self, state, streams=None) -> None:
        """Continues the comfort noise of the listed streams (None: slots 0 .. n - 1) from the counters `state`, uint32 [n]; 0 is fresh."""
        self._set_stage_state('comfort', (), np.uint32, 'uint32 counters', state, streams)

    def reset(self, stream_mask: Optional[np.ndarray] = None) -> None:
        ptr = None
        if stream_mask is not None:
            m = np.ascontiguousarray(stream_mask, dtype=np.uint8)
            if m.shape != (self.num_streams,):
                raise KoalaInvalidArgumentError("`stream_mask` must have one entry per stream")
            ptr = m.ctypes.data
        self._check(self._lib.pv_koala_batch_reset(self._handle, ptr), 'Reset failed')

    def set_stream(self, hip_stream: int) -> None:
        self._check(self._lib.pv_koala_batch_set_stream(self._handle, c_void_p(hip_stream)), 'set_stream failed')

    def synchronize(self) -> None:
        self._check(self._lib.pv_koala_batch_synchronize(self._handle), 'synchronize failed')

    def profile_enable(self, enable: bool = True) -> None:
        self._check(self._lib.pv_koala_batch_profile_enable(self._handle, 1 if enable else 0), 'profile failed')

    def profile_read(self):
        ms = (c_double * 5)()
        n = (c_int64 * 5)()
        self._check(self._lib.pv_koala_batch_profile_read(self._handle, ms, n), 'profile failed')
        return {k: {'ms': ms[i], 'launches': n[i]} for i, k in enumerate(KERNEL_CLASSES)}

    def debug_read(self, what: str, num_frames: int) -> np.ndarray:
        shapes = {'features': (0, (num_frames, self.num_streams, 257)), 'spectrum': (1, (num_frames, self.num_streams, 257, 2)),
                  'mask': (2, (num_frames, self.num_streams, 257)), 'hidden': (3, (8, self.num_streams, 271)),
                  'embed': (4, (num_frames, self.num_streams, 271)),
                  'route': (6, (4,)),  # developer library only: [route, features not stored, mask head fused, spectrum stored]
                  # developer library only: the same four, then the frames per time segment of the last analysis and of the last synthesis launch,
                  # and the call's synthesis launches (the slices of the layer pipeline, or one)
                  'segments': (6, (7,)),
                  'head_launches': (7, (1,))}  # developer library only: recurrent launches that carried their stage's narrow head
        code, shape = shapes[what]
        out = np.empty(shape, np.float32)
        n = self._lib.pv_koala_batch_debug_read(self._handle, code, out.ctypes.data, out.size)
        if n != out.size:
            raise KoalaError("debug_read(%s) returned %d, expected %d" % (what, n, out.size))
        return out

    def delete(self) -> None:
        if self._handle:
            self._lib.pv_koala_batch_delete(self._handle)
            self._handle = None
        for p in getattr(self, '_pinned', []):  # arrays from alloc_host() must not be used after this
            self._lib.pv_koala_batch_host_free(p)
        self._pinned = []

    def __del__(self):
        try:
            self.delete()
        except Exception:
            pass


__all__ = ['KoalaBatch', 'BatchCall', 'BatchPackets', 'BatchConfig', 'LevelSetting', 'LimiterSetting', 'ComfortSetting', 'PRECISION_FP32', 'PRECISION_BF16', 'KERNEL_CLASSES']
