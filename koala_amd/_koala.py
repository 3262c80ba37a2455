"""
ctypes binding of the MI355X-native libpv_koala.so -- same surface as the reference binding
(reference binding/python/_koala.py: exceptions :18-84, Koala :87-312, list_hardware_devices :315-339).

Differences from the reference binding, on purpose:
  * an empty `device` raises KoalaInvalidArgumentError (the reference raises NameError, _koala.py:149);
  * a failing device listing raises the mapped KoalaError (the reference hits an unqualified name, :332);
  * `process` also accepts numpy int16 arrays and converts them without a per-sample Python loop.
"""

import math
import os
from ctypes import (POINTER, Structure, byref, c_char_p, c_float, c_int, c_int16, c_int32, c_short, c_void_p, cdll, sizeof)
from typing import Optional, Sequence

import numpy as np

from . import bands
from ._errors import *  # noqa: F401,F403  (re-exported: the reference keeps the exceptions in this module)
from ._errors import STATUS_TO_EXCEPTION as _STATUS_TO_EXCEPTION
from ._errors import KoalaInvalidArgumentError, KoalaIOError, PicovoiceStatuses



def load_library(library_path: str):
    """dlopen the HIP build; there is no fallback of any kind if it is missing."""
    if not os.path.exists(library_path):
        raise KoalaIOError("Could not find Koala's dynamic library at `%s`." % library_path)
    library = cdll.LoadLibrary(library_path)
    library.pv_set_sdk.argtypes = [c_char_p]
    library.pv_set_sdk.restype = None
    library.pv_get_error_stack.argtypes = [POINTER(POINTER(c_char_p)), POINTER(c_int)]
    library.pv_get_error_stack.restype = PicovoiceStatuses
    library.pv_free_error_stack.argtypes = [POINTER(c_char_p)]
    library.pv_free_error_stack.restype = None
    library.pv_koala_version.argtypes = []
    library.pv_koala_version.restype = c_char_p
    return library


def fetch_error_stack(library) -> Sequence[str]:
    ref = POINTER(c_char_p)()
    depth = c_int()
    status = library.pv_get_error_stack(byref(ref), byref(depth))
    if status is not PicovoiceStatuses.SUCCESS:
        raise _STATUS_TO_EXCEPTION[status](message='Unable to get Koala error state')
    stack = [ref[i].decode('utf-8') for i in range(depth.value)]
    library.pv_free_error_stack(ref)
    return stack


def raise_status(library, status: PicovoiceStatuses, message: str) -> None:
    raise _STATUS_TO_EXCEPTION[status](message=message, message_stack=fetch_error_stack(library))


def attenuation_limit_to_gain(db) -> np.ndarray:
    """Attenuation limit(s) in dB -> minimum mask gain(s), float32, same shape: `None` or `inf` = unlimited = gain 0, 0 dB = bypass = gain
    1, otherwise float32(10 ** (-db / 20)) computed in double precision.  Negative or NaN limits raise ValueError."""
    a = np.asarray(np.inf if db is None else db, dtype=np.float64)
    if np.isnan(a).any() or (a < 0).any():
        raise ValueError("an attenuation limit is a number of dB >= 0 (None or inf: unlimited)")
    flat = [0.0 if math.isinf(v) else 10.0 ** (-v / 20.0) for v in a.ravel().tolist()]
    return np.array(flat, np.float64).reshape(a.shape).astype(np.float32)


class Koala(object):
    """One 16 kHz mono stream of the noise suppressor; `process` consumes and returns 256-sample frames."""

    PicovoiceStatuses = PicovoiceStatuses
    _PICOVOICE_STATUS_TO_EXCEPTION = _STATUS_TO_EXCEPTION

    class CKoala(Structure):
        pass

    def __init__(self, access_key: str, model_path: str, device: str, library_path: str) -> None:
        """
        :param access_key: kept for API compatibility; must be a non-empty string (no licence check is made).
        :param model_path: path of a KNS1 parameter file.
        :param device: `best`, `gpu` or `gpu:${GPU_INDEX}`.  `cpu` / `cpu:${NUM_THREADS}` parse but are refused.
        :param library_path: path of libpv_koala.so.
        """
        if not isinstance(access_key, str) or len(access_key) == 0:
            raise KoalaInvalidArgumentError("`access_key` should be a non-empty string.")
        if not os.path.exists(model_path):
            raise KoalaIOError("Could not find model file at `%s`." % model_path)
        if not isinstance(device, str) or len(device) == 0:
            raise KoalaInvalidArgumentError("`device` should be a non-empty string.")

        library = load_library(library_path)
        library.pv_set_sdk('python'.encode('utf-8'))
        self._library = library

        library.pv_koala_init.argtypes = [c_char_p, c_char_p, c_char_p, POINTER(POINTER(self.CKoala))]
        library.pv_koala_init.restype = PicovoiceStatuses
        self._handle = POINTER(self.CKoala)()
        status = library.pv_koala_init(access_key.encode(), model_path.encode(), device.encode(), byref(self._handle))
        if status is not PicovoiceStatuses.SUCCESS:
            raise_status(library, status, 'Initialization failed')

        self._delete_func = library.pv_koala_delete
        self._delete_func.argtypes = [POINTER(self.CKoala)]
        self._delete_func.restype = None

        library.pv_koala_delay_sample.argtypes = [POINTER(self.CKoala), POINTER(c_int32)]
        library.pv_koala_delay_sample.restype = PicovoiceStatuses
        delay = c_int32()
        status = library.pv_koala_delay_sample(self._handle, delay)
        if status is not PicovoiceStatuses.SUCCESS:
            self.delete()
            raise_status(library, status, 'Failed to get delay samples')
        self._delay_sample = delay.value

        self._process_func = library.pv_koala_process
        self._process_func.argtypes = [POINTER(self.CKoala), POINTER(c_short), POINTER(c_short)]
        self._process_func.restype = PicovoiceStatuses
        self._reset_func = library.pv_koala_reset
        self._reset_func.argtypes = [POINTER(self.CKoala)]
        self._reset_func.restype = PicovoiceStatuses

        self._set_min_gain_func = library.pv_koala_set_min_gain
        self._set_min_gain_func.argtypes = [POINTER(self.CKoala), c_float]
        self._set_min_gain_func.restype = PicovoiceStatuses
        self._get_min_gain_func = library.pv_koala_get_min_gain
        self._get_min_gain_func.argtypes = [POINTER(self.CKoala), POINTER(c_float)]
        self._get_min_gain_func.restype = PicovoiceStatuses

        self._process_report_func = library.pv_koala_process_report
        self._process_report_func.argtypes = [POINTER(self.CKoala), POINTER(c_short), POINTER(c_short), POINTER(c_float)]
        self._process_report_func.restype = PicovoiceStatuses

        self._sample_rate = library.pv_sample_rate()
        self._frame_length = library.pv_koala_frame_length()
        self._version = library.pv_koala_version().decode('utf-8')
        self._frame_type = c_short * self._frame_length

    def process(self, pcm: Sequence[int]) -> Sequence[int]:
        """
        One frame in, one (delayed) enhanced frame out.

        :param pcm: `frame_length` 16-bit samples, consecutive with the previous call unless `reset()` was called.
        :return: the enhanced samples that lie `delay_sample` behind the input, as a list of ints.
        """
        if len(pcm) != self._frame_length:
            raise KoalaInvalidArgumentError(
                "Length of input frame %d does not match required frame length %d" % (len(pcm), self._frame_length))
        if hasattr(pcm, 'ctypes') and getattr(pcm, 'dtype', None) == 'int16' and pcm.flags['C_CONTIGUOUS']:
            frame = pcm.ctypes.data_as(POINTER(c_short))
        else:
            frame = self._frame_type(*pcm)
        enhanced = self._frame_type()
        status = self._process_func(self._handle, frame, enhanced)
        if status is not PicovoiceStatuses.SUCCESS:
            raise_status(self._library, status, 'Processing failed')
        return list(enhanced)

    def process_with_report(self, pcm: Sequence[int]):
        """`process()` that also returns the frame's report (an extension: include/pv_koala_batch.h, pv_koala_process_report): a float32
        array [4] = e_in, e_out, mask_sum, 0 -- what came in, what goes out and how far the mask was open (koala_amd.report).  Calls with and
        without a report may be mixed; the samples are the same either way.

        :return: (enhanced samples as a list of ints, report)
        """
        if len(pcm) != self._frame_length:
            raise KoalaInvalidArgumentError(
                "Length of input frame %d does not match required frame length %d" % (len(pcm), self._frame_length))
        if hasattr(pcm, 'ctypes') and getattr(pcm, 'dtype', None) == 'int16' and pcm.flags['C_CONTIGUOUS']:
            frame = pcm.ctypes.data_as(POINTER(c_short))
        else:
            frame = self._frame_type(*pcm)
        enhanced = self._frame_type()
        report = np.zeros(4, np.float32)
        status = self._process_report_func(self._handle, frame, enhanced, report.ctypes.data_as(POINTER(c_float)))
        if status is not PicovoiceStatuses.SUCCESS:
            raise_status(self._library, status, 'Processing failed')
        return list(enhanced), report

    def reset(self) -> None:
        """Back to the state of a new instance; call between non-consecutive pieces of audio."""
        status = self._reset_func(self._handle)
        if status is not PicovoiceStatuses.SUCCESS:
            raise_status(self._library, status, 'Reset failed')

    def set_min_gain(self, gain: float) -> None:
        """Minimum mask gain in [0, 1] from the next frame on (an extension: include/pv_koala_batch.h, pv_koala_set_min_gain): 0 = no
        limit, 1 = bypass with unchanged latency, in between no bin is attenuated by more than -20 log10(gain) dB.  The stream's
        adapted state is not disturbed; `reset()` does not change the limit."""
        status = self._set_min_gain_func(self._handle, float(gain))
        if status is not PicovoiceStatuses.SUCCESS:
            raise_status(self._library, status, 'set_min_gain failed')

    def set_attenuation_limit(self, db: Optional[float]) -> None:
        """`set_min_gain` in dB: at most `db` dB of suppression (None or inf: unlimited; 0: bypass)."""
        self.set_min_gain(float(attenuation_limit_to_gain(db)))

    def min_gain(self) -> float:
        gain = c_float()
        status = self._get_min_gain_func(self._handle, byref(gain))
        if status is not PicovoiceStatuses.SUCCESS:
            raise_status(self._library, status, 'min_gain failed')
        return gain.value

    def set_band_profile(self, floor=None, ceiling=None) -> None:
        """Per-bin floor and ceiling on the mask from the next frame on (an extension: include/pv_koala_batch.h,
        pv_koala_set_band_profile): float32 [257] each, values in [0, 1], floor <= ceiling; None: zeros / ones -- `set_band_profile()`
        restores the neutral profile.  koala_amd.bands builds curves and states the rule.  `reset()` does not change the profile."""
        try:
            lo, hi = bands.check(floor, ceiling)
        except ValueError as e:
            raise KoalaInvalidArgumentError(str(e))
        fn = self._library.pv_koala_set_band_profile
        fn.argtypes, fn.restype = [POINTER(self.CKoala), c_void_p, c_void_p], PicovoiceStatuses
        status = fn(self._handle, lo.ctypes.data, hi.ctypes.data)
        if status is not PicovoiceStatuses.SUCCESS:
            raise_status(self._library, status, 'set_band_profile failed')

    def set_level(self, setting) -> None:
        """The output leveller from the next frame on (an extension: include/pv_koala_batch.h, pv_koala_set_level): a
        koala_amd.level.Setting (koala_amd.level.settings(target_dbfs=-23, ...)) or None for off.  `reset()` makes its state fresh and
        leaves the setting."""
        from ._batch import LevelSetting
        s = LevelSetting.of(setting)
        fn = self._library.pv_koala_set_level
        fn.argtypes, fn.restype = [POINTER(self.CKoala), c_void_p], PicovoiceStatuses
        status = fn(self._handle, byref(s))
        if status is not PicovoiceStatuses.SUCCESS:
            raise_status(self._library, status, 'set_level failed')

    def set_limiter(self, setting) -> None:
        """The peak limiter from the next frame on (an extension: include/pv_koala_batch.h, pv_koala_set_limiter): a
        koala_amd.limiter.Setting (koala_amd.limiter.settings(ceiling_dbfs=-1, release_ms=50)) or None for off.  `reset()` sets its gain
        to 1 and leaves the setting."""
        from ._batch import LimiterSetting
        s = LimiterSetting.of(setting)
        fn = self._library.pv_koala_set_limiter
        fn.argtypes, fn.restype = [POINTER(self.CKoala), c_void_p], PicovoiceStatuses
        status = fn(self._handle, byref(s))
        if status is not PicovoiceStatuses.SUCCESS:
            raise_status(self._library, status, 'set_limiter failed')

    def limiter(self):
        """The koala_amd.limiter.Setting in force."""
        from ._batch import LimiterSetting
        s = LimiterSetting(sizeof(LimiterSetting))
        fn = self._library.pv_koala_get_limiter
        fn.argtypes, fn.restype = [POINTER(self.CKoala), c_void_p], PicovoiceStatuses
        status = fn(self._handle, byref(s))
        if status is not PicovoiceStatuses.SUCCESS:
            raise_status(self._library, status, 'limiter failed')
        return s.setting()

    def set_comfort_noise(self, amplitude=None, seed=None, on=True) -> None:
        """Comfort noise from the next frame on (an extension: include/pv_koala_batch.h, pv_koala_set_comfort_noise): `amplitude` float32
        [257], finite and >= 0 (koala_amd.comfort.curve(-60) builds one; None: keep the curve), `seed` a uint32 (None: keep the seed, 0 on
        a new handle); `on=False` switches it off.  `reset()` makes the frame counter 0 and leaves the setting."""
        from . import comfort
        from ._batch import ComfortSetting
        try:
            amp = None if amplitude is None else comfort.check(amplitude)
        except (ValueError, TypeError) as e:
            raise KoalaInvalidArgumentError(str(e))
        s = ComfortSetting(sizeof(ComfortSetting), 1 if on else 0, (self.comfort_noise()[1] if seed is None else int(seed)) & 0xFFFFFFFF)
        fn = self._library.pv_koala_set_comfort_noise
        fn.argtypes, fn.restype = [POINTER(self.CKoala), c_void_p, c_void_p], PicovoiceStatuses
        status = fn(self._handle, byref(s), None if amp is None else amp.ctypes.data)
        if status is not PicovoiceStatuses.SUCCESS:
            raise_status(self._library, status, 'set_comfort_noise failed')

    def comfort_noise(self):
        """(on, seed, amplitude float32 [257]) in force."""
        from ._batch import ComfortSetting
        s, amp = ComfortSetting(sizeof(ComfortSetting)), np.empty(257, np.float32)
        fn = self._library.pv_koala_get_comfort_noise
        fn.argtypes, fn.restype = [POINTER(self.CKoala), c_void_p, c_void_p], PicovoiceStatuses
        status = fn(self._handle, byref(s), amp.ctypes.data)
        if status is not PicovoiceStatuses.SUCCESS:
            raise_status(self._library, status, 'comfort_noise failed')
        return bool(s.on), int(s.seed), amp

    def level(self):
        """The koala_amd.level.Setting in force."""
        from ._batch import LevelSetting
        s = LevelSetting(sizeof(LevelSetting))
        fn = self._library.pv_koala_get_level
        fn.argtypes, fn.restype = [POINTER(self.CKoala), c_void_p], PicovoiceStatuses
        status = fn(self._handle, byref(s))
        if status is not PicovoiceStatuses.SUCCESS:
            raise_status(self._library, status, 'level failed')
        return s.setting()

    def band_profile(self):
        """(floor, ceiling) in force, float32 [257] each."""
        lo, hi = np.empty(bands.NUM_BINS, np.float32), np.empty(bands.NUM_BINS, np.float32)
        fn = self._library.pv_koala_get_band_profile
        fn.argtypes, fn.restype = [POINTER(self.CKoala), c_void_p, c_void_p], PicovoiceStatuses
        status = fn(self._handle, lo.ctypes.data, hi.ctypes.data)
        if status is not PicovoiceStatuses.SUCCESS:
            raise_status(self._library, status, 'band_profile failed')
        return lo, hi

    def delete(self) -> None:
        """Releases the native stream."""
        self._delete_func(self._handle)
        self._handle = None

    @property
    def sample_rate(self) -> int:
        return self._sample_rate

    @property
    def frame_length(self) -> int:
        return self._frame_length

    @property
    def delay_sample(self) -> int:
        """Shift, in samples, between the input stream and the output stream."""
        return self._delay_sample

    @property
    def version(self) -> str:
        return self._version

    def _get_error_stack(self) -> Sequence[str]:
        return fetch_error_stack(self._library)


def list_hardware_devices(library_path: str) -> Sequence[str]:
    library = load_library(library_path)
    fn = library.pv_koala_list_hardware_devices
    fn.argtypes = [POINTER(POINTER(c_char_p)), POINTER(c_int32)]
    fn.restype = PicovoiceStatuses
    devices = POINTER(c_char_p)()
    count = c_int32()
    status = fn(byref(devices), byref(count))
    if status is not PicovoiceStatuses.SUCCESS:
        raise _STATUS_TO_EXCEPTION[status](message='`pv_koala_list_hardware_devices` failed.')
    result = [devices[i].decode() for i in range(count.value)]
    free = library.pv_koala_free_hardware_devices
    free.argtypes = [POINTER(c_char_p), c_int32]
    free.restype = None
    free(devices, count.value)
    return result


from . import _errors  # noqa: E402

__all__ = ['Koala', 'attenuation_limit_to_gain', 'list_hardware_devices', 'load_library', 'fetch_error_stack', 'raise_status'] + [
    n for n in _errors.__all__ if n != 'STATUS_TO_EXCEPTION']
