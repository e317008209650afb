"""The one loader of the tests' host builds (tests/<dirname>/, built by tests/host_build.mk): the shared library for ctypes and, where a
directory has one, the driver as a stand-alone program under the address and undefined-behaviour sanitizers.  Every target is named to
make, so loading a library never builds the sanitized program.  Test infrastructure: no product code is imported here.
"""
import ctypes
import os
import subprocess

TESTS = os.path.dirname(os.path.abspath(__file__))


def _make(dirname, target):
    d = os.path.join(TESTS, dirname)
    subprocess.run(["make", "-s", "-C", d, target], check=True, stdout=subprocess.DEVNULL)
    return os.path.join(d, target)


def load(dirname):
    """build tests/<dirname>/_build/lib<dirname>.so and load it -> ctypes.CDLL"""
    return ctypes.CDLL(_make(dirname, "_build/lib%s.so" % dirname))


def sanitized_program(dirname):
    """build the driver of tests/<dirname> with its own main under the sanitizers -> its path"""
    return _make(dirname, "_build/%s_san" % dirname)


def run_sanitized(dirname, timeout=120):
    """build that program and run it as a child process -> CompletedProcess (text, output captured)"""
    return subprocess.run([sanitized_program(dirname)], capture_output=True, text=True, timeout=timeout)


def ptr(a):
    """a numpy array's data as a void pointer; None stays None"""
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)
