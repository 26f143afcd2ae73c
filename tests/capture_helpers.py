"""The hipGraph plumbing of the capture tests (tests/test_fp32_capture.py, tests/test_half16_capture.py, tests/test_capture_base.py): the
graph API straight from the HIP runtime the library is linked against (no torch: a second HIP runtime in the process is not needed)."""
import ctypes as C


def ok(rc):
    assert rc == 0, f"HIP runtime call failed: {rc}"


class Graph:
    """one stream, one graph captured on it in global mode, one executable graph"""

    def __init__(self):
        self.rt = C.CDLL("libamdhip64.so")
        self.stream, self.graph, self.gexec = C.c_void_p(), C.c_void_p(), C.c_void_p()
        ok(self.rt.hipStreamCreate(C.byref(self.stream)))

    def begin(self):
        ok(self.rt.hipStreamBeginCapture(self.stream, 0))                  # hipStreamCaptureModeGlobal

    def end(self):
        """hipStreamEndCapture's own return code: a test of a refused call looks at it"""
        return self.rt.hipStreamEndCapture(self.stream, C.byref(self.graph))

    def record(self, enqueue):
        self.begin()
        try:
            enqueue(self.stream)
        finally:                                                           # a failed call must not leave the stream capturing
            rc = self.end()
        ok(rc)
        ok(self.rt.hipGraphInstantiate(C.byref(self.gexec), self.graph, None, None, 0))

    def capture(self, enqueue):
        enqueue(self.stream)                                           # one ordinary call first
        ok(self.rt.hipStreamSynchronize(self.stream))
        self.record(enqueue)

    def sync(self):
        ok(self.rt.hipStreamSynchronize(self.stream))

    def replay(self):
        ok(self.rt.hipGraphLaunch(self.gexec, self.stream))
        ok(self.rt.hipStreamSynchronize(self.stream))

    def close(self, lib=None):
        """lib: the stream goes through clv_stream_destroy, which also drops the library's scratch of the stream"""
        if self.gexec:
            ok(self.rt.hipGraphExecDestroy(self.gexec))
        if self.graph:
            ok(self.rt.hipGraphDestroy(self.graph))
        if lib is not None:
            assert lib.clv_stream_destroy(self.stream) == 0
        else:
            ok(self.rt.hipStreamDestroy(self.stream))


def fresh_graph(lib):
    """a Graph on a stream of which the library knows nothing.  The runtime hands the handle of a destroyed stream out again, and a test
    that closed with plain hipStreamDestroy leaves the library's scratch entry of that handle behind; clv_stream_destroy drops it.  So:
    destroy through the library, create again, until a handle comes back that was cleaned this way."""
    cleaned = set()
    for _ in range(32):
        g = Graph()
        if g.stream.value in cleaned:
            return g
        cleaned.add(g.stream.value)
        assert lib.clv_stream_destroy(g.stream) == 0
    return Graph()                                                         # no handle came back in 32 tries: take what comes
