"""
Live-stream noise suppression: the reference's microphone demo (demo/python/koala_demo_mic.py:75-121: a recorder hands
over one frame at a time, every frame goes through `Koala.process`, the enhanced -- and optionally the original --
audio is appended to a WAV file until Ctrl+C) restated on koala_amd.  This environment has no capture device and no
`pvrecorder`, so the frame source is a byte stream of raw 16 kHz mono int16 PCM: stdin by default (e.g.
`arecord -f S16_LE -r 16000 -c 1 -t raw | python -m koala_amd.demo.koala_demo_stream --output_path out.wav`), or a WAV
file replayed with `--realtime` pacing.  One frame per call = the hipGraph latency path (BASELINE configs[4]).

    python -m koala_amd.demo.koala_demo_stream --output_path clean.wav < noisy.raw
    python -m koala_amd.demo.koala_demo_stream --input_path noisy.wav --realtime --output_path clean.wav --reference_output_path in.wav
"""
import argparse
import contextlib
import struct
import sys
import time
import wave

import numpy as np

import koala_amd


def frames_from_raw(stream, frame_length):
    """Yields int16 frames from a binary stream; a trailing partial frame is zero-padded (the recorder never makes one)."""
    nbytes = 2 * frame_length
    while True:
        buf = stream.read(nbytes)
        if not buf:
            return
        while len(buf) < nbytes:  # pipes deliver short reads
            more = stream.read(nbytes - len(buf))
            if not more:
                break
            buf += more
        frame = np.zeros(frame_length, np.int16)
        got = np.frombuffer(buf[:len(buf) // 2 * 2], dtype='<i2')
        frame[:len(got)] = got
        yield frame
        if len(buf) < nbytes:
            return


def frames_from_wav(path, frame_length, sample_rate):
    with wave.open(path, 'rb') as f:
        if f.getframerate() != sample_rate or f.getnchannels() != 1 or f.getsampwidth() != 2:
            raise ValueError('`%s` must be %d Hz, single-channel, 16-bit PCM' % (path, sample_rate))
        pcm = np.frombuffer(f.readframes(f.getnframes()), dtype=np.int16)
    for start in range(0, len(pcm), frame_length):
        frame = np.zeros(frame_length, np.int16)
        chunk = pcm[start:start + frame_length]
        frame[:len(chunk)] = chunk
        yield frame


def run_in_packets(args):
    """--packet-ms: the stream arrives in packets of 10 or 20 ms, not in frames, and goes through a packet handle (one stream of
    `koala_amd.create_batch(..., packet_samples=N)`): every packet returns as many samples as it brought, `delay_sample` later.
    --meter and --reference_output_path work as with frames: the report rows are those of the frames a packet completes."""
    import os
    from koala_amd import report
    rate = 16000  # the rate the handle is made at; the packet length follows from it
    batch = koala_amd.create_batch(args.access_key, 1, precision=args.precision or os.environ.get('KOALA_AMD_PRECISION', 'fp32'),
                                   model_path=args.model_path, device=args.device, library_path=args.library_path,
                                   sample_rate=rate, packet_samples=rate * args.packet_ms // 1000)
    n, lat, packets, samples, frames = batch.packet_samples, [], 0, 0, 0
    meter = []  # report rows since the last printed line
    source = frames_from_wav(args.input_path, n, batch.sample_rate) if args.input_path else frames_from_raw(sys.stdin.buffer, n)
    batch.set_attenuation_limit(args.attenuation_limit_db)
    set_band_profile(batch, args)
    set_level(batch, args)
    set_comfort(batch, args)
    t_start = time.perf_counter()
    try:
        with contextlib.ExitStack() as stack:
            def open_wav(path):
                w = stack.enter_context(wave.open(path, 'wb'))
                w.setnchannels(1), w.setsampwidth(2), w.setframerate(batch.sample_rate)
                return w
            out = open_wav(args.output_path)
            ref = open_wav(args.reference_output_path) if args.reference_output_path else None
            print('Listening in packets of %d ms (%d samples; a frame is %d)... (press Ctrl+C to stop)' % (args.packet_ms, n, batch.frame_length))
            for packet in source:
                if args.realtime:
                    due = t_start + samples / batch.sample_rate
                    if due > time.perf_counter():
                        time.sleep(due - time.perf_counter())
                t0 = time.perf_counter()
                if args.meter > 0:
                    enhanced, done, rows = batch.process_packets(packet[None], [n], report=True)
                    enhanced = enhanced[0]
                else:
                    enhanced = batch.process_packets(packet[None], [n])[0]
                lat.append(time.perf_counter() - t0)
                if args.meter > 0:
                    for row in rows[0, :int(done[0])]:
                        frames += 1
                        meter.append(row)
                        if len(meter) == args.meter:
                            total = np.sum(np.array(meter, np.float64), axis=0)  # (energies and mask sums add up over the N frames)
                            total[2] /= len(meter)
                            print('frame %6d  in %7.1f dBFS  suppression %6.1f dB  mean gain %.3f' %
                                  (frames, report.input_dbfs(total / [len(meter), len(meter), 1, 1]), report.suppression_db(total),
                                   report.mean_gain(total)))
                            meter = []
                out.writeframes(enhanced.astype('<i2').tobytes())
                if ref is not None:
                    ref.writeframes(packet.astype('<i2').tobytes())
                packets, samples = packets + 1, samples + n
    except KeyboardInterrupt:
        print('Stopping...')
    finally:
        delay, rate = batch.delay_sample, batch.sample_rate
        batch.delete()
    if packets:
        a = np.array(lat) * 1e6
        print('%d packets (%.2f s of audio); process_packets() latency p50 %.0f us, p99 %.0f us; delay %d samples' %
              (packets, samples / float(rate), np.percentile(a, 50), np.percentile(a, 99), delay))
    return 0


def run_raw_format(args):
    """--sample_format: raw samples of that format (s16: little-endian int16; f32: little-endian float32 in [-1, 1); ulaw / alaw: G.711
    bytes) on stdin at --sample_rate, the enhanced stream in the same format on stdout, through one stream of a packet handle
    (`koala_amd.create_batch(..., packet_samples=N, sample_format=...)`: the conversion runs on the device).  Telephony, for instance:
    `... | koala_demo_stream.py --sample_format ulaw --sample_rate 8000 --packet-ms 20 | ...`.  Messages go to stderr."""
    import os
    from koala_amd import formats
    rate, dt = args.sample_rate, np.dtype(formats.dtype(args.sample_format)).newbyteorder('<')
    n = rate * (args.packet_ms or 20) // 1000
    batch = koala_amd.create_batch(args.access_key, 1, precision=args.precision or os.environ.get('KOALA_AMD_PRECISION', 'fp32'),
                                   model_path=args.model_path, device=args.device, library_path=args.library_path,
                                   sample_rate=rate, packet_samples=n, sample_format=args.sample_format)
    batch.set_attenuation_limit(args.attenuation_limit_db)
    set_band_profile(batch, args)
    set_level(batch, args)
    set_comfort(batch, args)
    samples = 0
    try:
        while True:
            buf = sys.stdin.buffer.read(n * dt.itemsize)
            got = np.frombuffer(buf[:len(buf) // dt.itemsize * dt.itemsize], dtype=dt)
            if got.size == 0:
                break
            packet = np.zeros((1, n), formats.dtype(args.sample_format))
            packet[0, :got.size] = got
            enhanced = batch.process_packets(packet, [got.size])
            sys.stdout.buffer.write(enhanced[0, :got.size].astype(dt).tobytes())
            sys.stdout.buffer.flush()
            samples += got.size
    except KeyboardInterrupt:
        pass
    finally:
        delay = batch.delay_sample
        batch.delete()
    print('%d samples of %s at %d Hz; delay %d samples' % (samples, args.sample_format, rate, delay), file=sys.stderr)
    return 0


def run_channels(args):
    """--channels C: C interleaved channels (L R L R ...) through the C streams of one group of a packet handle
    (`koala_amd.create_batch(..., packet_samples=N, channels=C)`: split and joined on the device), at --sample_rate, for instance
    `--sample_rate 44100 --channels 2`.  With --input_path / --output_path: a C-channel 16-bit WAV of that rate in, one out.  Otherwise raw
    interleaved samples of --sample_format (s16 by default) on stdin, the enhanced stream in the same form on stdout.  Every channel is
    enhanced on its own unless --link is given (`channel_link='max'`: one mask per group, C = 2, 4 or 8).  Messages go to stderr."""
    import os
    from koala_amd import formats
    C, rate, fmt = args.channels, args.sample_rate, args.sample_format or 's16'
    for name, v in (('--meter', args.meter), ('--realtime', args.realtime), ('--reference_output_path', args.reference_output_path)):
        if v:
            raise ValueError('%s: not available with --channels' % name)
    if (args.input_path is None) != (args.output_path is None):
        raise ValueError('--channels: give both --input_path and --output_path (WAV files) or neither (raw samples on stdin and stdout)')
    if args.input_path and fmt != 's16':
        raise ValueError('--channels: WAV files are 16-bit PCM; --sample_format %s is for raw samples on stdin and stdout' % fmt)
    dt = np.dtype(formats.dtype(fmt)).newbyteorder('<')
    n = rate * (args.packet_ms or 20) // 1000
    with contextlib.ExitStack() as stack:
        if args.input_path:
            src = stack.enter_context(wave.open(args.input_path, 'rb'))
            if (src.getnchannels(), src.getsampwidth(), src.getframerate()) != (C, 2, rate):
                raise ValueError('%s: expected a %d-channel 16-bit WAV at %d Hz' % (args.input_path, C, rate))
            dst = stack.enter_context(wave.open(args.output_path, 'wb'))
            dst.setnchannels(C), dst.setsampwidth(2), dst.setframerate(rate)
            read, write = (lambda: src.readframes(n)), dst.writeframes
        else:
            read = lambda: sys.stdin.buffer.read(n * C * dt.itemsize)
            write = lambda b: (sys.stdout.buffer.write(b), sys.stdout.buffer.flush())
        batch = koala_amd.create_batch(args.access_key, C, precision=args.precision or os.environ.get('KOALA_AMD_PRECISION', 'fp32'),
                                       model_path=args.model_path, device=args.device, library_path=args.library_path,
                                       sample_rate=rate, packet_samples=n, sample_format=fmt, channels=C,
                                       channel_link='max' if args.link else None)
        batch.set_attenuation_limit(args.attenuation_limit_db)
        if args.link and (args.highpass is not None or args.max_depth_db is not None):
            raise ValueError('--link: not available with --highpass or --max_depth_db yet (the library refuses a band profile on linked channels)')
        set_band_profile(batch, args)
        set_level(batch, args)
        set_comfort(batch, args)
        samples = 0
        try:
            while True:
                buf = read()
                got = np.frombuffer(buf[:len(buf) // (C * dt.itemsize) * (C * dt.itemsize)], dtype=dt)  # whole samples of all channels
                if got.size == 0:
                    break
                packet = np.zeros((1, n * C), formats.dtype(fmt))
                packet[0, :got.size] = got
                enhanced = batch.process_packets(packet, [got.size // C] * C)
                write(enhanced[0, :got.size].astype(dt).tobytes())
                samples += got.size // C
        except KeyboardInterrupt:
            pass
        finally:
            delay = batch.delay_sample
            batch.delete()
    print('%d samples of %d channels of %s at %d Hz; delay %d samples' % (samples, C, fmt, rate, delay), file=sys.stderr)
    return 0


def set_band_profile(handle, args):
    """--highpass HZ: nothing below HZ comes out (a ceiling, koala_amd.bands.highpass); --max_depth_db DB: no bin is suppressed by more than
    DB dB (a floor, koala_amd.bands.depth_limit_db)"""
    if args.highpass is None and args.max_depth_db is None:
        return
    from koala_amd import bands
    ceiling = None if args.highpass is None else bands.highpass(args.highpass)
    floor = None if args.max_depth_db is None else bands.depth_limit_db([(0.0, args.max_depth_db)])
    if floor is not None and ceiling is not None:
        floor = np.minimum(floor, ceiling)  # (below the high-pass the ceiling wins)
    handle.set_band_profile(floor, ceiling)


def set_comfort(handle, args):
    """--comfort_noise DBFS: white comfort noise of DBFS dB RMS where the mask removes everything (koala_amd.comfort.curve(DBFS))"""
    if args.comfort_noise is None:
        return
    if args.link or args.sample_rate in (44100, 22050):
        raise ValueError('--comfort_noise: not available with --link nor at 44100 / 22050 Hz yet (the library refuses the call)')
    from koala_amd import comfort
    handle.set_comfort_noise(comfort.curve(args.comfort_noise))


def set_level(handle, args):
    """--level [DBFS]: the output leveller (koala_amd.level.settings(target_dbfs=DBFS), -23 when no value is given): speech is brought
    towards DBFS by a gain that adapts on speech frames only.  --limiter DBFS: the peak limiter behind it
    (koala_amd.limiter.settings(ceiling_dbfs=DBFS)): no inner sample above DBFS, instant attack, 50 ms linear release; without it
    saturation alone bounds the levelled samples"""
    for name, value in (('--level', args.level), ('--limiter', args.limiter)):
        if value is not None and (args.link or args.sample_rate in (44100, 22050)):
            raise ValueError('%s: not available with --link nor at 44100 / 22050 Hz yet (the library refuses the call)' % name)
    if args.level is not None:
        from koala_amd import level
        handle.set_level(level.settings(target_dbfs=args.level))
    if args.limiter is not None:
        from koala_amd import limiter
        handle.set_limiter(limiter.settings(ceiling_dbfs=args.limiter))


def run_high_band(args):
    """--high_band: a mono 16-bit WAV at --sample_rate 32000 or 48000 through one stream of a frame handle with the high-band carry
    (`koala_amd.create_batch(..., sample_rate=rate, high_band='carry')`): the band above the 16 kHz call's is delayed like the call, scaled
    by a broadband gain from the call's masks and added back, so full-band audio stays full-band.  Frame by frame, --input_path to
    --output_path; the output is `delay_sample` samples late."""
    import os
    rate = args.sample_rate
    if rate not in (32000, 48000):
        raise ValueError('--high_band: --sample_rate must be 32000 or 48000 (lower rates have no band to carry; the others are not available yet)')
    for name, v in (('--meter', args.meter), ('--packet-ms', args.packet_ms), ('--sample_format', args.sample_format),
                    ('--highpass', args.highpass is not None), ('--max_depth_db', args.max_depth_db is not None), ('--level', args.level is not None),
                    ('--limiter', args.limiter is not None)):
        if v:
            raise ValueError('%s: not available with --high_band' % name)
    if args.input_path is None or args.output_path is None:
        raise ValueError('--high_band: give --input_path and --output_path (mono 16-bit WAV files at --sample_rate)')
    batch = koala_amd.create_batch(args.access_key, 1, precision=args.precision or os.environ.get('KOALA_AMD_PRECISION', 'fp32'),
                                   model_path=args.model_path, device=args.device, library_path=args.library_path,
                                   sample_rate=rate, high_band='carry')
    batch.set_attenuation_limit(args.attenuation_limit_db)
    frames = 0
    try:
        with wave.open(args.output_path, 'wb') as out:
            out.setnchannels(1), out.setsampwidth(2), out.setframerate(rate)
            for frame in frames_from_wav(args.input_path, batch.frame_length, rate):
                out.writeframes(batch.process(frame[None])[0].astype('<i2').tobytes())
                frames += 1
    finally:
        delay = batch.delay_sample
        batch.delete()
    print('%d frames at %d Hz with the high-band carry; delay %d samples' % (frames, rate, delay), file=sys.stderr)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(description='frame-by-frame noise suppression of a live PCM stream')
    ap.add_argument('--access_key', default='koala-amd', help='accepted for interface compatibility; not checked')
    ap.add_argument('--input_path', default=None, help='WAV file to replay instead of raw PCM on stdin')
    ap.add_argument('--output_path', default=None, help='WAV file for the enhanced audio')
    ap.add_argument('--reference_output_path', default=None, help='WAV file for the unprocessed input')
    ap.add_argument('--model_path', default=None)
    ap.add_argument('--library_path', default=None)
    ap.add_argument('--device', default=None)
    ap.add_argument('--precision', default=None, choices=['fp32', 'bf16'],
                    help='mask network arithmetic (default: the library default, fp32, or $KOALA_AMD_PRECISION)')
    ap.add_argument('--realtime', action='store_true', help='pace a replayed file at 16 ms per frame, like a recorder')
    ap.add_argument('--attenuation_limit_db', type=float, default=None,
                    help='suppress by at most this many dB (0: bypass with unchanged latency; default: unlimited)')
    ap.add_argument('--highpass', type=float, default=None, metavar='HZ',
                    help='band profile: let nothing out below HZ (rumble, 50 / 60 Hz hum), a raised-cosine edge 62.5 Hz wide')
    ap.add_argument('--max_depth_db', type=float, default=None, metavar='DB',
                    help='band profile: suppress no bin by more than DB dB (a floor on the mask)')
    ap.add_argument('--comfort_noise', type=float, default=None, metavar='DBFS',
                    help='comfort noise: fill what the mask removes with white noise of DBFS dB RMS (for instance -60)')
    ap.add_argument('--level', type=float, nargs='?', const=-23.0, default=None, metavar='DBFS',
                    help='output leveller: bring speech towards DBFS (default -23) with a speech-gated automatic gain')
    ap.add_argument('--limiter', type=float, default=None, metavar='DBFS',
                    help='peak limiter: no sample of the 16 kHz output above DBFS (for instance -1), instant attack, linear release')
    ap.add_argument('--meter', type=int, default=0, metavar='N',
                    help='every N frames print input level (dBFS), suppression (dB) and mean mask gain, from the frame report')
    ap.add_argument('--packet-ms', dest='packet_ms', type=int, default=0, choices=[10, 20],
                    help='feed the stream in packets of this many ms through a packet handle instead of in 16 ms frames')
    ap.add_argument('--sample_format', default=None, choices=['s16', 'f32', 'ulaw', 'alaw'],
                    help='raw samples of this format on stdin and stdout at --sample_rate, through a packet handle that converts on the device')
    ap.add_argument('--sample_rate', type=int, default=16000, choices=[8000, 12000, 16000, 22050, 24000, 32000, 44100, 48000],
                    help='with --sample_format: the stream\'s rate (22050 and 44100 imply --sample_format s16 when none is given)')
    ap.add_argument('--channels', type=int, default=1, choices=range(1, 9), metavar='C',
                    help='C interleaved channels (raw on stdin and stdout, or C-channel WAV files) at --sample_rate through a packet '
                         'handle that splits and joins on the device; every channel is enhanced on its own')
    ap.add_argument('--link', action='store_true',
                    help="with --channels 2, 4 or 8: one mask per group, the max of the channels' own (the stereo image does not move)")
    ap.add_argument('--high_band', action='store_true',
                    help='with --sample_rate 32000 or 48000 and WAV files: carry the band above 8 kHz around the 16 kHz call (a frame handle)')
    ap.add_argument('--show_devices', action='store_true')
    args = ap.parse_args(argv)

    if args.show_devices:
        print('\n'.join(koala_amd.available_devices(library_path=args.library_path)))
        return 0
    if args.high_band:
        if args.channels != 1:
            raise ValueError('--high_band: not available with --channels in this demo')
        return run_high_band(args)
    if args.channels != 1:
        return run_channels(args)
    if args.sample_rate in (22050, 44100):
        # no frame exists at these rates: the raw packet path (stdin -> stdout) is the only one, and it has no files, meter or pacing
        given = [name for name, v in (('--input_path', args.input_path), ('--output_path', args.output_path),
                                      ('--reference_output_path', args.reference_output_path), ('--meter', args.meter),
                                      ('--realtime', args.realtime)) if v]
        if given:
            raise ValueError('%s: not available at --sample_rate %d, where the stream is raw samples on stdin and stdout '
                             '(--sample_format, s16 by default)' % (', '.join(given), args.sample_rate))
        if args.sample_format is None:
            args.sample_format = 's16'
    if args.sample_format is not None:
        return run_raw_format(args)
    if args.output_path is None:
        raise ValueError('Missing required argument --output_path')
    for p in (args.output_path, args.reference_output_path):
        if p is not None and not p.lower().endswith('.wav'):
            raise ValueError('Given output paths must have WAV file extension')

    if args.packet_ms:
        return run_in_packets(args)
    if args.precision is not None:
        import os
        os.environ['KOALA_AMD_PRECISION'] = args.precision
    koala = koala_amd.create(access_key=args.access_key, model_path=args.model_path, device=args.device,
                             library_path=args.library_path)
    koala.set_attenuation_limit(args.attenuation_limit_db)
    set_band_profile(koala, args)
    set_level(koala, args)
    set_comfort(koala, args)
    print('Koala version: %s' % koala.version)
    n = koala.frame_length
    source = (frames_from_wav(args.input_path, n, koala.sample_rate) if args.input_path
              else frames_from_raw(sys.stdin.buffer, n))
    lat = []
    frames = 0
    meter = []  # report rows since the last printed line
    t_start = time.perf_counter()
    try:
        with contextlib.ExitStack() as stack:
            def open_wav(path):
                w = stack.enter_context(wave.open(path, 'wb'))
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(koala.sample_rate)
                return w
            out = open_wav(args.output_path)
            ref = open_wav(args.reference_output_path) if args.reference_output_path else None
            print('Listening... (press Ctrl+C to stop)')
            for frame in source:
                if args.realtime:
                    due = t_start + frames * n / koala.sample_rate
                    now = time.perf_counter()
                    if due > now:
                        time.sleep(due - now)
                t0 = time.perf_counter()
                if args.meter > 0:
                    enhanced, row = koala.process_with_report(frame)
                else:
                    enhanced = koala.process(frame)
                lat.append(time.perf_counter() - t0)
                if args.meter > 0:
                    meter.append(row)
                    if len(meter) == args.meter:
                        from koala_amd import report
                        total = np.sum(np.array(meter, np.float64), axis=0)  # (energies and mask sums add up over the N frames)
                        total[2] /= len(meter)
                        print('frame %6d  in %7.1f dBFS  suppression %6.1f dB  mean gain %.3f' %
                              (frames + 1, report.input_dbfs(total / [len(meter), len(meter), 1, 1]), report.suppression_db(total),
                               report.mean_gain(total)))
                        meter = []
                out.writeframes(struct.pack('%dh' % n, *enhanced))
                if ref is not None:
                    ref.writeframes(struct.pack('%dh' % n, *[int(v) for v in frame]))
                frames += 1
    except KeyboardInterrupt:
        print('Stopping...')
    finally:
        koala.delete()
    if frames:
        a = np.array(lat) * 1e6
        print('%d frames (%.2f s of audio); process() latency p50 %.0f us, p99 %.0f us; delay %d samples' %
              (frames, frames * n / 16000.0, np.percentile(a, 50), np.percentile(a, 99), 256))
        print('Real time factor: %.4f' % (float(np.sum(lat)) / (frames * n / 16000.0)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
