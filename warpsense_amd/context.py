"""Context: device and HIP stream of the library, and the reference's pause / cleanup (src/warpsense/cuda/cleanup.cu)."""
from __future__ import annotations

import ctypes as C
import threading

from . import _lib
from ._lib import check


class Context:
    """One per process and GPU: device + HIP stream (the reference uses the implicit CUDA context)."""

    _default = None
    _lock = threading.Lock()

    def __init__(self, device_id: int = -1):
        self._L = _lib.load()
        h = C.c_void_p()
        check(self._L.ws_ctx_create(int(device_id), C.byref(h)), "ws_ctx_create")
        self.handle = h

    @classmethod
    def default(cls) -> "Context":
        with cls._lock:
            if cls._default is None:
                cls._default = cls()
            return cls._default

    def set_stream(self, hip_stream_ptr):
        check(self._L.ws_ctx_set_stream(self.handle, C.c_void_p(hip_stream_ptr) if hip_stream_ptr else None),
              "ws_ctx_set_stream")

    def use_torch_stream(self):
        """Run the library's work on torch's CURRENT stream, so that torch operations (copies of the 44 sums, RCCL
        collectives) and the library's kernels are ordered by the stream alone.  The C ABI takes a hipStream_t and reads
        NULL as "the context's own stream", so torch's legacy default stream (handle 0) cannot be named there: in that case
        a new stream is created and made torch's current stream (for this thread) first."""
        import torch
        cur = torch.cuda.current_stream()
        if cur.cuda_stream == 0:
            # SIDE EFFECT, for the calling thread: torch's current stream becomes a new stream (restored by
            # restore_torch_stream() / close()).  The new stream first waits for everything already queued on the default
            # stream -- uploads or preprocessing the caller enqueued there -- so nothing queued earlier can race with later work.
            self._torch_prev_stream = cur
            new = torch.cuda.Stream()
            new.wait_stream(cur)
            torch.cuda.set_stream(new)
            cur = new
        self._torch_stream = cur  # keep it alive
        self.set_stream(cur.cuda_stream)

    def restore_torch_stream(self):
        """Undo use_torch_stream()'s stream switch: the library goes back to its own stream (after the work queued so far)
        and torch's current stream for this thread is the one it was before."""
        prev = getattr(self, "_torch_prev_stream", None)
        if prev is None:
            return
        import torch
        cur = getattr(self, "_torch_stream", None)
        if self.handle:
            self.set_stream(None)  # synchronises the stream it leaves
        if cur is not None:
            prev.wait_stream(cur)
        torch.cuda.set_stream(prev)
        self._torch_prev_stream = None
        self._torch_stream = None

    def sync(self):
        check(self._L.ws_sync(self.handle), "ws_sync")

    # hipEvent timing of kernel classes (bench.py)
    def prof_enable(self, mask: int):
        check(self._L.ws_prof_enable(self.handle, int(mask)), "ws_prof_enable")

    def prof_reset(self):
        check(self._L.ws_prof_reset(self.handle), "ws_prof_reset")

    def prof_read(self, cls: int):
        ms, n = C.c_double(0), C.c_int64(0)
        check(self._L.ws_prof_read(self.handle, int(cls), C.byref(ms), C.byref(n)), "ws_prof_read")
        return ms.value, n.value

    def close(self):
        if self.handle:
            try:
                self.restore_torch_stream()
            except Exception:  # noqa: BLE001 - closing must not fail on a torch that is already shutting down
                pass
            self._L.ws_ctx_destroy(self.handle)
            self.handle = None


def pause(ctx: Context | None = None):
    """cuda::pause() — cleanup.cu:3-6."""
    (ctx or Context.default()).sync()


def cleanup():
    """cuda::cleanup() — cleanup.cu:8-11.  Resets the device: every handle becomes invalid."""
    check(_lib.load().ws_device_reset(), "ws_device_reset")
    Context._default = None
