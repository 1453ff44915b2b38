"""Held pages of a payload stream (pbsgpu_stream_hold / _release / _held / _upload_new2_device / _copy_device; DESIGN.md
§19) without a GPU: the header section and its feature macro, every new symbol exported and bound, the Python, Go and
C++ surfaces, and the argument checks that come before the stream is looked at."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pbsgpu_stream_hold", "pbsgpu_stream_release", "pbsgpu_stream_held", "pbsgpu_stream_upload_new2_device",
           "pbsgpu_stream_copy_device")


@pytest.fixture(scope="module")
def L():
    from pbs_plus_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_header_section_and_its_define():
    hdr = _read("include", "pbsgpu.h")
    assert re.search(r"^#define PBSGPU_HAS_STREAM_UPLOAD 1\b", hdr, flags=re.M)
    assert re.search(r"^#define PBSGPU_ABI_VERSION 5\b", hdr, flags=re.M)       # additive: the version stays
    # the section stands behind the held pages of the ring and in front of the next one
    ring, here, nxt = hdr.index("PBSGPU_HAS_RING_UPLOAD 1"), hdr.index("PBSGPU_HAS_STREAM_UPLOAD 1"), hdr.index("whole-stream SHA-256 batch")
    assert ring < hdr.index("pbsgpu_ring_copy_device(") < here < nxt
    for name in SYMBOLS:
        assert re.search(r"^int %s\(" % name, hdr[here:nxt], flags=re.M), name
    # the engine options are frozen: the switch is a call on the stream
    opts = hdr[hdr.index("typedef struct pbsgpu_engine_options"):hdr.index("} pbsgpu_engine_options;")]
    assert "hold" not in opts


def test_new_names_are_exported_and_bound(L):
    from pbs_plus_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (pbsgpu_[a-z0-9_]+)", out))
    for name in SYMBOLS:
        assert name in exported, name
        assert name in _lib.SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    # the stream call takes the ring call's arguments without the stream number
    ring = _lib.SYMBOLS["pbsgpu_ring_upload_new2_device"][1]
    assert _lib.SYMBOLS["pbsgpu_stream_upload_new2_device"][1] == ring[:2] + ring[3:]


def test_python_cpp_and_go_surfaces():
    from pbs_plus_amd import PayloadStream

    for m in ("upload_new2", "release", "held", "copy"):
        assert callable(getattr(PayloadStream, m)), m
    assert inspect.signature(PayloadStream.__init__).parameters["hold"].default is False
    assert list(inspect.signature(PayloadStream.copy).parameters)[1:] == ["position", "length", "dst"]
    hpp = _read("include", "pbsgpu.hpp")
    go = _read("go", "pbsgpu", "pbsgpu.go")
    fb = _read("go", "pbsgpu", "fallback.go")
    writer = hpp[hpp.index("class PayloadWriter"):hpp.index("class PageRing")]
    for name in SYMBOLS:
        assert name + "(" in writer, name
        assert re.search(r"\bC\.%s\(" % name, go), name
    for sig in (r"^func \(s \*Stream\) Hold\(", r"^func \(s \*Stream\) UploadNew2\(", r"^func \(s \*Stream\) Release\(",
                r"^func \(s \*Stream\) Held\(", r"^func \(s \*Stream\) Copy\("):
        assert re.search(sig, go, flags=re.M), sig
        assert re.search(sig, fb, flags=re.M), sig


def test_null_arguments_are_invalid(L):
    """The checks that come before the stream is looked at: a NULL stream, and NULL where a result must go."""
    from pbs_plus_amd import RECORD_DTYPE, _lib

    E = _lib.E_INVALID
    fake = C.cast(C.create_string_buffer(4096), C.c_void_p)  # never dereferenced: the NULL argument is found first
    recs = np.zeros(2, dtype=RECORD_DTYPE)
    offs = np.zeros(2, dtype=np.uint64)
    first, pages, free, used = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint64()
    st = _lib.DedupStats()
    assert L.pbsgpu_stream_hold(None) == E
    assert L.pbsgpu_stream_release(None, 0) == E
    assert L.pbsgpu_stream_held(None, C.byref(first), C.byref(pages), C.byref(free)) == E
    assert L.pbsgpu_stream_held(fake, None, C.byref(pages), C.byref(free)) == E
    assert L.pbsgpu_stream_held(fake, C.byref(first), None, None) == E
    up = L.pbsgpu_stream_upload_new2_device
    rp, op, un, sp = recs.ctypes.data, offs.ctypes.data, C.byref(used), C.byref(st)
    assert up(None, fake, rp, 2, 1, 0, None, 0, None, op, None, None, None, un, sp, None) == E
    assert up(fake, None, rp, 2, 1, 0, None, 0, None, op, None, None, None, un, sp, None) == E
    assert up(fake, fake, None, 2, 1, 0, None, 0, None, op, None, None, None, un, sp, None) == E
    assert up(fake, fake, rp, 2, 1, 0, None, 0, None, None, None, None, None, un, sp, None) == E
    assert up(fake, fake, rp, 2, 1, 0, None, 0, None, op, None, None, None, None, sp, None) == E
    assert up(fake, fake, rp, 2, 1, 0, None, 0, None, op, None, None, None, un, None, None) == E
    assert up(fake, fake, rp, 2, 1, 2, None, 0, None, op, None, None, None, un, sp, None) == E      # an unknown flag bit
    assert up(fake, fake, rp, 2, 1, 0, None, 64, None, op, None, None, None, un, sp, None) == E     # a capacity and no dst
    assert L.pbsgpu_stream_copy_device(None, 0, 16, fake) == E
    assert L.pbsgpu_stream_copy_device(fake, 0, 16, None) == E
    assert L.pbsgpu_stream_copy_device(fake, (1 << 64) - 8, 16, fake) == E                       # the range wraps
