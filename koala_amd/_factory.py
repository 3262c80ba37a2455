"""Factory functions (mirrors reference binding/python/_factory.py:27-76, plus `create_batch`)."""

from typing import Optional, Sequence

from ._batch import KoalaBatch
from ._koala import Koala, list_hardware_devices
from ._util import default_library_path, default_model_path


def create(
        access_key: str,
        model_path: Optional[str] = None,
        device: Optional[str] = None,
        library_path: Optional[str] = None) -> Koala:
    """
    Single-stream engine, drop-in for `pvkoala.create`.

    :param access_key: non-empty string, not verified.
    :param model_path: KNS1 parameter file; default: the packaged `lib/koala_params.kns`.
    :param device: `best` (default), `gpu` or `gpu:${GPU_INDEX}`.
    :param library_path: libpv_koala.so; default: the in-tree HIP build.
    """
    return Koala(
        access_key=access_key,
        model_path=default_model_path() if model_path is None else model_path,
        device='best' if device is None else device,
        library_path=default_library_path() if library_path is None else library_path)


def create_batch(
        access_key: str,
        num_streams: int,
        max_frames_per_call: int = 1,
        precision: str = 'fp32',
        model_path: Optional[str] = None,
        device: Optional[str] = None,
        library_path: Optional[str] = None,
        sample_rate: int = 16000,
        packet_samples: int = 0,
        sample_format: str = 's16',
        channels: int = 1,
        channel_link: Optional[str] = None,
        high_band: Optional[str] = None,
        band_profile=None,
        level=None,
        comfort_noise=None,
        limiter=None) -> KoalaBatch:
    """`num_streams` independent streams advancing together on one GPU (see KoalaBatch), at 8000, 12000, 16000, 24000, 32000 or 48000 Hz.
    `packet_samples=N` makes a packet handle: streams that take and deliver any number of samples, up to N, per call
    (`KoalaBatch.process_packets`; `max_frames_per_call` is then derived from N).
    `sample_format`: 's16' (default), 'f32', 'ulaw' or 'alaw' -- the handle takes and delivers np.float32 or G.711 np.uint8 arrays,
    converted on the device (`koala_amd.formats` has the codecs).
    `channels=C` (2 ... 8): every array of samples is [num_streams / C, n * C], the C streams of a group interleaved (L R L R ...), split
    and joined on the device (`koala_amd.channels` has the layout); the streams stay independent, everything per stream stays [num_streams].
    `channel_link='max'` (`channels` 2, 4 or 8): the channels of a group share one mask, the max of their own, bin by bin
    (`KoalaBatch.set_channel_link`).
    `high_band='carry'` (a frame handle at 32000 or 48000 Hz): the band above the 16 kHz call's is carried around it and added back
    (`KoalaBatch.set_high_band`; `koala_amd.highband` has the rule).
    `band_profile=(floor, ceiling)`: a per-bin floor and ceiling on the mask of every stream (`KoalaBatch.set_band_profile`;
    `koala_amd.bands` builds the curves and has the rule).
    `level=koala_amd.level.settings(...)`: the output leveller on every stream, a speech-gated automatic gain behind the suppressor
    (`KoalaBatch.set_level`; `koala_amd.level` has the rule).
    `limiter=koala_amd.limiter.settings(ceiling_dbfs=-1)`: the peak limiter on every stream, a ceiling on the output with instant attack and
    linear release, behind the leveller (`KoalaBatch.set_limiter`; `koala_amd.limiter` has the rule).
    `comfort_noise=koala_amd.comfort.curve(-60)` (or a pair (curve, seed)): comfort noise on every stream, a shaped noise exactly where the
    mask removed energy (`KoalaBatch.set_comfort_noise`; `koala_amd.comfort` has the rule)."""
    return KoalaBatch(
        access_key=access_key,
        model_path=default_model_path() if model_path is None else model_path,
        device='best' if device is None else device,
        library_path=default_library_path() if library_path is None else library_path,
        num_streams=num_streams,
        max_frames_per_call=max_frames_per_call,
        precision=precision,
        sample_rate=sample_rate,
        packet_samples=packet_samples,
        sample_format=sample_format,
        channels=channels,
        channel_link=channel_link,
        high_band=high_band,
        band_profile=band_profile,
        level=level,
        comfort_noise=comfort_noise,
        limiter=limiter)


def available_devices(library_path: Optional[str] = None) -> Sequence[str]:
    """Every string that `create(device=...)` accepts on this machine ("gpu:0 - <name>", ...)."""
    return list_hardware_devices(library_path=default_library_path() if library_path is None else library_path)


__all__ = ['available_devices', 'create', 'create_batch']
