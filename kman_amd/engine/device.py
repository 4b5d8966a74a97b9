"""The device layer: one HIP context, its buffers and the scratch scope of a call."""

from __future__ import annotations

import ctypes
import os
from ctypes import byref, c_size_t, c_void_p
from typing import Optional, Tuple

import numpy as np

from .. import _native as N
from .. import phases


# text bytes per pipelined slice through the pinned stages: the file loader
# (parse_file), the writer (_format_dev) and the read cutter (cut_records)
_FMT_SLICE = 256 << 20


def host_threads() -> int:
    n = os.cpu_count() or 1
    return max(1, min(n, int(os.environ.get("KMAN_HOST_THREADS", "16"))))


class DeviceBuffer:
    """A device allocation owned by a :class:`Device`."""

    __slots__ = ("dev", "ptr", "nbytes")

    def __init__(self, dev: "Device", nbytes: int):
        self.dev = dev
        p = c_void_p()
        N.check(dev.ctx, N.lib().kman_malloc(dev.ctx, byref(p), max(1, int(nbytes))), "kman_malloc(%d)" % nbytes)
        self.ptr = p.value
        self.nbytes = int(nbytes)

    def free(self) -> None:
        if self.ptr and self.dev is not None and self.dev.ctx:
            N.lib().kman_free(self.dev.ctx, c_void_p(self.ptr))
        self.ptr = None

    def __del__(self):  # pragma: no cover - best effort at teardown
        try:
            self.free()
        except Exception:
            pass

    def offset(self, nbytes: int) -> int:
        return self.ptr + int(nbytes)


class Device:
    """One HIP context (stream, look-back scratch) on one GPU."""

    def __init__(self, device: int = 0):
        L = N.lib()
        ctx = c_void_p()
        rc = L.kman_create(int(device), byref(ctx))
        if rc != N.KMAN_OK:
            raise RuntimeError(
                "kman_create(device=%d) failed (%d): no usable MI355X/HIP device (%d visible)"
                % (device, rc, N.device_count())
            )
        self.ctx = ctx.value
        self.index = device
        self._fmt = None  # (cap, pinned stages) of the pipelined writer and the file loader
        phases.mark("device_init")

    def pinned_stages(self, cap: int, nb: int):
        """nb pinned host stages of >= cap bytes, kept across calls (a pinned
        allocation of a few hundred MB costs tens of ms: per call it was a
        large part of a bounded write): the pipelined writer's D2H stages and
        the chunked file loader's H2D stages.  Device memory is not held."""
        if self._fmt is not None and self._fmt[0] >= cap and len(self._fmt[1]) >= nb:
            return self._fmt[1]
        self._free_fmt()
        L = N.lib()
        stages = []
        try:
            for _ in range(nb):
                hp = c_void_p()
                N.check(self.ctx, L.kman_host_alloc(self.ctx, byref(hp), cap), "kman_host_alloc")
                stages.append(hp)
        except Exception:
            for hp in stages:
                L.kman_host_free(self.ctx, hp)
            raise
        self._fmt = (cap, stages)
        return stages

    def _free_fmt(self) -> None:
        if self._fmt is not None and self.ctx:
            L = N.lib()
            L.kman_copy_sync(self.ctx)
            for hp in self._fmt[1]:
                L.kman_host_free(self.ctx, hp)
        self._fmt = None

    def close(self) -> None:
        if self.ctx:
            self._free_fmt()
            N.lib().kman_destroy(c_void_p(self.ctx))
            self.ctx = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # -- memory
    def alloc(self, nbytes: int) -> DeviceBuffer:
        return DeviceBuffer(self, nbytes)

    def upload(self, buf: DeviceBuffer, data, offset: int = 0) -> None:
        mv = memoryview(data).cast("B")
        if offset + mv.nbytes > buf.nbytes:
            raise ValueError("upload overflows the device buffer")
        src = (ctypes.c_char * mv.nbytes).from_buffer_copy(mv) if mv.readonly else (ctypes.c_char * mv.nbytes).from_buffer(mv)
        N.check(self.ctx, N.lib().kman_memcpy_h2d(self.ctx, c_void_p(buf.ptr + offset), src, mv.nbytes), "h2d")

    def download(self, buf: DeviceBuffer, count: int, dtype, offset: int = 0) -> np.ndarray:
        out = np.empty(int(count), dtype=dtype)
        if out.nbytes:
            N.check(
                self.ctx,
                N.lib().kman_memcpy_d2h(self.ctx, out.ctypes.data_as(c_void_p), c_void_p(buf.ptr + offset), out.nbytes),
                "d2h",
            )
        return out

    def memset(self, buf: DeviceBuffer, value: int, nbytes: int, offset: int = 0) -> None:
        N.check(self.ctx, N.lib().kman_memset(self.ctx, c_void_p(buf.ptr + offset), value, nbytes), "memset")

    def sync(self) -> None:
        N.check(self.ctx, N.lib().kman_sync(self.ctx), "sync")

    def scratch(self) -> "Scratch":
        return Scratch(self)


def free_all(*bufs) -> None:
    """``free()`` of every buffer given that is not None (an object's own buffers)."""
    for b in bufs:
        if b is not None:
            b.free()


class Scratch:
    """The device buffers of one call, as a context manager: on exit, normal
    or by exception, every buffer still tracked is freed, the newest first.
    A ``free()`` that raises does not stop the others, and is raised only
    when no other exception is on its way."""

    def __init__(self, dev: Device):
        self.dev = dev
        self._bufs = []

    def alloc(self, nbytes: int) -> DeviceBuffer:
        return self.own(self.dev.alloc(nbytes))

    def own(self, buf):
        """Adopt a buffer made elsewhere (a table_index, a window_counts); returns it."""
        self._bufs.append(buf)
        return buf

    def keep(self, buf):
        """Stop tracking a buffer, the caller's from here on; returns it."""
        self._bufs = [b for b in self._bufs if b is not buf]
        return buf

    def __enter__(self) -> "Scratch":
        return self

    def __exit__(self, exc_type, exc, tb) -> bool:
        failed = None
        while self._bufs:
            try:
                self._bufs.pop().free()
            except Exception as e:
                failed = failed or e
        if failed is not None and exc_type is None:
            raise failed
        return False


_DEFAULT: Optional[Device] = None


def default_device() -> Device:
    """Process-wide device (LOCAL_RANK when launched one process per GPU)."""
    global _DEFAULT
    if _DEFAULT is None:
        _DEFAULT = Device(int(os.environ.get("KMAN_DEVICE", os.environ.get("LOCAL_RANK", "0"))))
    return _DEFAULT


def mem_info(dev: Device) -> Tuple[int, int]:
    """(free, total) HBM bytes of the device (kman_mem_info)."""
    f, t = c_size_t(0), c_size_t(0)
    N.check(dev.ctx, N.lib().kman_mem_info(dev.ctx, byref(f), byref(t)), "kman_mem_info")
    return int(f.value), int(t.value)


class BorrowedBuffer:
    """A device buffer that somebody else owns: ``ptr`` follows the owner's
    (None once the owner freed it) and ``free`` does nothing, so a view can be
    freed, or dropped, any number of times without touching the allocation."""

    __slots__ = ("_owner",)

    def __init__(self, owner: DeviceBuffer):
        self._owner = owner

    @property
    def ptr(self):
        return self._owner.ptr

    @property
    def nbytes(self) -> int:
        return self._owner.nbytes

    @property
    def dev(self):
        return self._owner.dev

    def free(self) -> None:
        pass

    def offset(self, nbytes: int) -> int:
        return self.ptr + int(nbytes)
