"""
The kernels' own source of koala_amd/csrc/kns_resample.hip and kns_highband.hip on the CPU (tests/highband_emulation: 256 OS threads a
workgroup, every array a heap allocation of exactly its documented size) as ONE stand-alone program under AddressSanitizer +
UndefinedBehaviorSanitizer, built once per session, and the comparison of what it writes with the numpy recipes
(tests/sample_rate_recipe.Stage, tests/high_band_recipe.HighBand) -- every comparison ==.  Shared by tests/test_sample_rate.py and
tests/test_high_band.py; not a test module.
"""
import os

import numpy as np

import sample_rate_recipe as srr
import sanitized_build
from conftest import ROOT
from high_band_recipe import Y_HIST, HighBand

CSRC = os.path.join(ROOT, 'koala_amd', 'csrc')
TYPES = {'i16': np.int16, 'u8': np.uint8, 'f32': np.float32, 'i32': np.int32}
# (U, D, q_frame) of both stages of all five rates: a frame is q_frame groups of D input and U output samples, 256 samples on its 16 kHz side
STAGE_CASES = [(rate, k) for rate in srr.RATES for k in (0, 1)]


def translation_unit(highband_text=None):
    """shim + the sample-rate and high-band sections of kns_kernels.h + the kernels of both files, cut in front of their launch_* functions
    + driver.  `highband_text`: another text in place of kns_highband.hip (a mutated scratch copy)."""
    src = os.path.join(ROOT, 'tests', 'highband_emulation')
    header = open(os.path.join(CSRC, 'kns_kernels.h')).read()
    section = (header[header.index('constexpr int kRate16k'):header.index('// ---- packet handles')] +
               header[header.index('constexpr int kHbYHist'):header.index('void launch_high_band(')])
    # (without the launchers' declarations, which name HIP types, and the one line that belongs to the stream records)
    section = '\n'.join(line for line in section.splitlines() if not line.startswith(('void launch_', 'KNS_HD size_t state_record_bytes'))) + '\n'
    rs = open(os.path.join(CSRC, 'kns_resample.hip')).read().replace('#include "kns_kernels.h"', '')
    rs = rs[:rs.index('void launch_resample(')] + '}\n'
    hb = highband_text if highband_text is not None else open(os.path.join(CSRC, 'kns_highband.hip')).read()
    hb = hb.replace('#include "kns_kernels.h"', '')
    hb = hb[:hb.index('void launch_high_band(')].replace('namespace kns {', 'namespace kns { namespace hbk {', 1) + '}}\n'
    return (open(os.path.join(src, 'shim.inc')).read() + 'namespace kns {\n' + section + '}\n' + rs + hb +
            open(os.path.join(src, 'driver.inc')).read())


_program = []


def program(tmp_path_factory):
    """the emulator, built at its first use"""
    if not _program:
        _program.append(sanitized_build.build_translation_unit(translation_unit(), tmp_path_factory.mktemp('highband_emulation'),
                                                               ['-ffp-contract=off']))
    return _program[0]


def records(path):
    """the driver's file -> [(name, array)] in the order written"""
    out, data, at = [], open(path, 'rb').read(), 0
    while at < len(data):
        end = data.index(b'\n', at)
        name, kind, n = data[at:end].decode().split()
        dt = np.dtype(TYPES[kind])
        at = end + 1 + int(n) * dt.itemsize
        out.append((name, np.frombuffer(data[end + 1:at], dt).copy()))
    assert at == len(data)
    return out


def run(exe, directory, *args):
    path = os.path.join(str(directory), 'emu_' + '_'.join(str(a) for a in args) + '.bin')
    got = sanitized_build.run(exe, *args, path)
    assert got.returncode == 0 and got.stdout.strip() == 'done' and not got.stderr.strip(), (got.returncode, got.stdout[-2000:], got.stderr[-6000:])
    return records(path)


class Reader:
    def __init__(self, recs):
        self.recs, self.at = recs, 0

    def take(self, name):
        got, a = self.recs[self.at]
        assert got == name, (got, name, self.at)
        self.at += 1
        return a

    def done(self):
        return self.at == len(self.recs)


def check_stage(exe, directory, rate, k):
    """one stage of a handle at `rate` (k = 0: the in-stage) == sample_rate_recipe.Stage call by call, flags frame by frame; -> calls"""
    (U, D), B = srr.STAGES[rate][k], 3
    qf = 256 // (D if k else U)
    r = Reader(run(exe, directory, 'rs', U, D, qf))
    ref = srr.Stage(B, max(U, D), U, D)
    H = ref.hist.shape[1]
    assert np.array_equal(r.take('taps'), ref.table)
    assert not r.take('state0').any() and not r.take('state1').any()  # the reset kernel, mask null, over both copies
    seen = []
    while not r.done():
        T = int(r.take('T')[0])
        mask, flags = r.take('mask'), r.take('flags').reshape(B, -1)
        x, y, state = r.take('in').reshape(B, T * qf * D), r.take('out').reshape(B, T * qf * U), r.take('state').reshape(B, H)
        ref.reset(mask)
        if flags.size:
            want = []
            for t in range(T):
                ref.reset(flags[:, t])
                want.append(ref.run(x[:, t * qf * D:(t + 1) * qf * D]))
            want = np.concatenate(want, axis=1)
        else:
            want = ref.run(x)
        assert np.array_equal(y, want), (rate, k, len(seen), np.argwhere(y != want)[:4].tolist())
        assert np.array_equal(state, ref.hist), (rate, k, len(seen))
        seen.append((T, bool(mask.any()), flags.copy()))
    return seen


def check_carry(exe, directory, rate):
    """the in-stage kernel and high_band_kernel<R> behind it == HighBand call by call, in samples and in all three state arrays; -> calls"""
    R, B = rate // 16000, 4
    r = Reader(run(exe, directory, 'hb', R))
    for _ in range(2):
        assert not r.take('xs0').any() and not r.take('ys0').any() and not r.take('ss0').any()  # the reset kernel, mask null
    ref, stage, seen = HighBand(B, rate), srr.Stage(B, R, 1, R), []
    while not r.done():
        T, link = int(r.take('T')[0]), int(r.take('link')[0])
        mask, flags, gains = r.take('mask'), r.take('flags').reshape(B, -1), r.take('gains')
        x, y, e = r.take('x').reshape(B, T * 256 * R), r.take('y').reshape(B, T * 256), r.take('E').reshape(B, T * 256 * R)
        rep, out = r.take('report').reshape(B, T, 4), r.take('out').reshape(B, T * 256 * R)
        xs, ys, ss = r.take('xs').reshape(B, Y_HIST * R), r.take('ys').reshape(B, Y_HIST), r.take('ss').reshape(B, 2)
        assert (rep[:, :, 2] >= 0).all() and (rep[:, :, 2] <= 257).all()
        fresh = mask.astype(bool) | (flags[:, 0] != 0 if flags.size else False)
        ref.reset(fresh), stage.reset(fresh)
        ref.C = link if link > 1 else 1
        assert np.array_equal(y, stage.run(x)), (rate, len(seen))
        want = ref.process(x, e, rep[:, :, 2], gains if gains.size else 0.0)
        assert np.array_equal(out, want), (rate, len(seen), np.argwhere(out != want)[:4].tolist())
        assert np.array_equal(xs, ref.x_hist) and np.array_equal(ys, ref.y_hist), (rate, len(seen))
        assert np.array_equal(ss.view(np.uint32), ref.sp.view(np.uint32)), (rate, len(seen), ss.tolist(), ref.sp.tolist())
        seen.append(dict(T=T, link=link, mask=bool(mask.any()), flags=bool(flags.size), gains=bool(gains.size), moved=int((out != e).sum()),
                         full=bool(np.abs(x[0].astype(int)).max() > 32000 and np.abs(e[0].astype(int)).max() > 32000)))
    return seen
