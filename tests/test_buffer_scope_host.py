"""CPU, no library: device.BufferScope over a stub context whose alloc returns recording stub buffers -- what is released, in
which order, and which exception the caller sees."""
import importlib

import pytest

from helpers import PKG

D = importlib.import_module(PKG + ".device")


class StubBuffer:
    def __init__(self, log, name, nbytes, fail=False):
        self.log, self.name, self.nbytes, self.fail, self.ptr = log, name, nbytes, fail, 0x1000

    def free(self):
        self.log.append(self.name)
        self.ptr = None
        if self.fail:
            raise OSError("free of %s failed" % self.name)


class StubIndex:
    def __init__(self, log, name):
        self.log, self.name = log, name

    def close(self):
        self.log.append(self.name)


class StubContext:
    """alloc() hands out StubBuffers named b0, b1, ...; the names in `failing` raise from free()"""

    def __init__(self, failing=()):
        self.log, self.sizes, self.failing = [], [], set(failing)

    def alloc(self, nbytes):
        name = "b%d" % len(self.sizes)
        self.sizes.append(nbytes)
        return StubBuffer(self.log, name, nbytes, name in self.failing)


def test_release_on_a_normal_exit_in_reverse_order():
    ctx = StubContext()
    with D.BufferScope(ctx) as B:
        bufs = [B.alloc(8), B.alloc(16), B.alloc(24)]
        assert ctx.log == [] and ctx.sizes == [8, 16, 24]
    assert ctx.log == ["b2", "b1", "b0"]
    assert all(b.ptr is None for b in bufs)


def test_release_when_the_body_raises():
    ctx = StubContext()
    with pytest.raises(KeyError, match="body"):
        with D.BufferScope(ctx) as B:
            B.alloc(8), B.alloc(8)
            raise KeyError("body")
    assert ctx.log == ["b1", "b0"]


def test_the_body_exception_wins_over_a_failing_free_and_everything_is_still_released():
    ctx = StubContext(failing={"b1"})
    with pytest.raises(KeyError, match="body"):
        with D.BufferScope(ctx) as B:
            B.alloc(8), B.alloc(8), B.alloc(8)
            raise KeyError("body")
    assert ctx.log == ["b2", "b1", "b0"]


def test_a_failing_free_is_raised_when_nothing_else_is_in_flight_after_the_rest_is_released():
    ctx = StubContext(failing={"b1", "b0"})
    with pytest.raises(OSError, match="free of b1 failed"):      # the first failure, in release order
        with D.BufferScope(ctx) as B:
            B.alloc(8), B.alloc(8), B.alloc(8)
    assert ctx.log == ["b2", "b1", "b0"]


def test_an_adopted_object_goes_before_the_buffers_it_was_created_after():
    ctx = StubContext()
    with D.BufferScope(ctx) as B:
        B.alloc(8)
        index = StubIndex(ctx.log, "index")
        assert B.adopt(index) is index
        B.alloc(8)
    assert ctx.log == ["b1", "index", "b0"]


def test_close_twice_is_harmless_and_the_scope_can_be_used_again():
    ctx = StubContext()
    B = D.BufferScope(ctx)
    B.alloc(8)
    B.close()
    B.close()
    assert ctx.log == ["b0"]
    B.alloc(8)
    B.close()
    assert ctx.log == ["b0", "b1"]


def test_sizes_pass_through_unchanged():
    ctx = StubContext()
    with D.BufferScope(ctx) as B:
        assert B.alloc(0).nbytes == 0 and B.alloc(5).nbytes == 5
    assert ctx.sizes == [0, 5]
