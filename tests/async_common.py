"""What tests/test_gpu_async.py needs from the HIP runtime itself: caller streams, caller device buffers and the in-flight query.

A thin ctypes wrapper over libamdhip64 (the library under test is never asked about its own frames here):

* stream(slot, nonblocking): caller streams, created lazily, in two slots - AT MOST TWO CALLER STREAMS EXIST AT ANY TIME, which together
  with the context's own stream stays below four hardware queues.  destroy_streams() drains and destroys them.
* DeviceFrame(W, H, frames, floats): a float buffer (frames * H * W * floats) and an RGBA8 buffer (frames * H * W) in HBM, both
  pre-filled with the byte 0xA5 - a pixel the call failed to write or to clear shows as 0xA5A5A5A5 - and read back after a synchronize.
* in_flight(stream): hipStreamQuery == hipErrorNotReady.
"""
import ctypes as C
import os

import numpy as np

HIP_SUCCESS = 0
HIP_ERROR_NOT_READY = 600
STREAM_DEFAULT, STREAM_NON_BLOCKING = 0, 1  # hipStreamCreateWithFlags
H2D, D2H = 1, 2  # hipMemcpyKind
FILL = 0xA5

_hip = None
_streams = {}  # slot -> (handle, flags)


def hip():
    global _hip
    if _hip is None:
        h = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
        h.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
        for f in (h.hipStreamDestroy, h.hipStreamQuery, h.hipStreamSynchronize, h.hipFree):
            f.argtypes = [C.c_void_p]
        h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        h.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip = h
    return _hip


def _ok(rc, what):
    assert rc == HIP_SUCCESS, "%s failed: hipError %d" % (what, rc)


def stream(slot, nonblocking=True):
    """The caller stream of slot 0 or 1 as an integer (what binding.Context takes as stream=), created on first use with the given flag.
    A slot that holds a stream of the other flag is drained, destroyed and created anew."""
    assert slot in (0, 1), "two caller streams at most"
    flags = STREAM_NON_BLOCKING if nonblocking else STREAM_DEFAULT
    if slot in _streams and _streams[slot][1] != flags:
        _destroy(slot)
    if slot not in _streams:
        s = C.c_void_p()
        _ok(hip().hipStreamCreateWithFlags(C.byref(s), flags), "hipStreamCreateWithFlags")
        assert s.value
        _streams[slot] = (s.value, flags)
    return _streams[slot][0]


def _destroy(slot):
    s, _ = _streams.pop(slot)
    _ok(hip().hipStreamSynchronize(s), "hipStreamSynchronize")
    _ok(hip().hipStreamDestroy(s), "hipStreamDestroy")


def destroy_streams():
    for slot in list(_streams):
        _destroy(slot)


def query(s):
    """hipStreamQuery's code: HIP_SUCCESS (everything enqueued on s is complete) or HIP_ERROR_NOT_READY."""
    return int(hip().hipStreamQuery(s))


def in_flight(s):
    return query(s) == HIP_ERROR_NOT_READY


def synchronize(s):
    _ok(hip().hipStreamSynchronize(s), "hipStreamSynchronize")


def to_device(ptr, a):
    """A blocking copy of a host array to a device pointer (an integer)."""
    a = np.ascontiguousarray(a)
    _ok(hip().hipMemcpy(C.c_void_p(ptr), a.ctypes.data_as(C.c_void_p), a.nbytes, H2D), "hipMemcpy")


class DeviceFrame:
    """Caller-owned output buffers of `frames` frames of W x H: .rgb (frames * H * W * floats float32) and .rgba8 (frames * H * W
    uint32), device pointers as integers, every byte 0xA5 until a call writes it.  read() copies both back (after a synchronize: a
    blocking hipMemcpy on the null stream does not wait for a non-blocking stream)."""

    def __init__(self, W, H, frames=1, floats=3):
        self.shape = ((frames,) if frames > 1 else ()) + (H, W)
        self.floats = floats
        self.nbytes = frames * H * W * floats * 4
        self.nbytes8 = frames * H * W * 4
        self._p, self._p8 = C.c_void_p(), C.c_void_p()
        _ok(hip().hipMalloc(C.byref(self._p), self.nbytes), "hipMalloc")
        try:
            _ok(hip().hipMalloc(C.byref(self._p8), self.nbytes8), "hipMalloc")
            _ok(hip().hipMemset(self._p, FILL, self.nbytes), "hipMemset")
            _ok(hip().hipMemset(self._p8, FILL, self.nbytes8), "hipMemset")
            _ok(hip().hipDeviceSynchronize(), "hipDeviceSynchronize")  # the fill is complete before any stream writes the buffers
        except BaseException:
            self.free()
            raise
        self.rgb, self.rgba8 = self._p.value, self._p8.value

    def read(self):
        rgb = np.empty(self.shape + (self.floats,), np.float32)
        rgba8 = np.empty(self.shape, np.uint32)
        _ok(hip().hipMemcpy(rgb.ctypes.data_as(C.c_void_p), self._p, self.nbytes, D2H), "hipMemcpy")
        _ok(hip().hipMemcpy(rgba8.ctypes.data_as(C.c_void_p), self._p8, self.nbytes8, D2H), "hipMemcpy")
        return rgb, rgba8

    def free(self):
        for p in (self._p, self._p8):
            if p.value:
                hip().hipFree(p)
                p.value = None
