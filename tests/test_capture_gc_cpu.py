"""Stream captures run with Python's cyclic garbage collector out of the way (usflows_amd/_ext.py: capture_without_gc): a
collection inside a capture destroys the CUDAGraph objects of dead flows, and on ROCm that destructor synchronises the device,
which a capture in progress forbids -- the process aborts."""
import gc
import glob
import os
import re

import pytest

from usflows_amd import _ext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_collector_is_off_inside_and_back_on_behind():
    class Node:
        pass
    a, b = Node(), Node()
    a.other, b.other = b, a
    seen = []
    a.mark = type("Mark", (), {"__del__": lambda self: seen.append(gc.isenabled())})()
    del a, b
    assert gc.isenabled()
    with _ext.capture_without_gc():
        assert seen == [True]               # the dead cycle was collected on the way in, before the collector was switched off
        assert not gc.isenabled()
        with _ext.capture_without_gc():     # (nested: the inner one leaves it off)
            assert not gc.isenabled()
        assert not gc.isenabled()
    assert gc.isenabled()
    with pytest.raises(ValueError):
        with _ext.capture_without_gc():
            raise ValueError("a capture that fails")
    assert gc.isenabled()
    gc.disable()
    try:
        with _ext.capture_without_gc():
            pass
        assert not gc.isenabled()           # it was off before: it stays off
    finally:
        gc.enable()


def test_every_capture_of_the_package_uses_it():
    sites = 0
    for path in glob.glob(os.path.join(ROOT, "usflows_amd", "*.py")):
        for line in open(path):
            if re.match(r"\s*with\b.*torch\.cuda\.graph\(", line):
                sites += 1
                assert "_ext.capture_without_gc()" in line.split("torch.cuda.graph(")[0], (path, line.strip())
    assert sites == 3
