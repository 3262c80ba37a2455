"""
The route numbers that the GPU tests assert (tests/gpu_kit.py, ROUTE_*) are the engine's: names and values of `enum Route` in
koala_amd/csrc/kns_engine.cpp, read as text.  No GPU, no build.
"""
import os
import re

import gpu_kit
from conftest import ROOT


def test_the_kits_route_table_is_the_engines_enum():
    with open(os.path.join(ROOT, 'koala_amd', 'csrc', 'kns_engine.cpp')) as f:
        found = re.findall(r'^enum Route \{(.*)\};$', f.read(), re.M)
    assert len(found) == 1, found
    enum = {}
    for entry in found[0].split(','):
        name, value = re.fullmatch(r'\s*kRoute(\w+) = (\d+)\s*', entry).groups()
        # kRouteSmallSteps -> ROUTE_SMALL_STEPS; the kit calls kRouteChunkedResets ROUTE_RESETS
        kit = 'ROUTE_' + re.sub(r'(?<!^)(?=[A-Z])', '_', name).upper()
        enum['ROUTE_RESETS' if kit == 'ROUTE_CHUNKED_RESETS' else kit] = int(value)
    kit = {name: value for name, value in vars(gpu_kit).items() if name.startswith('ROUTE_')}
    assert len(enum) == len(found[0].split(',')) and kit == enum, (kit, enum)
