"""The scratch scope of kman_amd.engine.device on a fake device: what it
frees, in which order, and what a failing free() does."""

from __future__ import annotations

import pytest

from kman_amd.engine.device import Scratch


class _Buf:
    def __init__(self, log, name, fail=False):
        self.log, self.name, self.fail = log, name, fail

    def free(self):
        self.log.append(self.name)
        if self.fail:
            raise RuntimeError("free of %s failed" % self.name)


class _Dev:
    """alloc() makes buffers named a0, a1, .. that record their free() in `log`."""

    def __init__(self, failing=()):
        self.log, self.made, self.failing = [], 0, set(failing)

    def alloc(self, nbytes):
        name = "a%d" % self.made
        self.made += 1
        return _Buf(self.log, name, name in self.failing)

    def scratch(self):
        return Scratch(self)


def test_freed_in_reverse_order_on_normal_exit():
    dev = _Dev()
    with dev.scratch() as s:
        a, b, c = s.alloc(8), s.alloc(8), s.alloc(8)
        assert (a.name, b.name, c.name) == ("a0", "a1", "a2")
        assert dev.log == []
    assert dev.log == ["a2", "a1", "a0"]


def test_freed_in_reverse_order_on_an_exception():
    dev = _Dev()
    with pytest.raises(KeyError, match="inside"):
        with dev.scratch() as s:
            s.alloc(8), s.alloc(8)
            raise KeyError("inside")
    assert dev.log == ["a1", "a0"]


def test_keep_hands_the_buffer_back_and_own_adopts_one():
    dev = _Dev()
    theirs = _Buf(dev.log, "theirs")
    with dev.scratch() as s:
        a = s.alloc(8)
        assert s.own(theirs) is theirs
        res = s.alloc(8)
        assert s.keep(res) is res
        assert s.keep(None) is None  # (an optional result that was not made)
    assert dev.log == ["theirs", a.name]
    assert res.name == "a1" and "a1" not in dev.log


def test_keep_on_the_error_path_still_frees_the_rest():
    dev = _Dev()
    with pytest.raises(ValueError):
        with dev.scratch() as s:
            kept = s.keep(s.alloc(8))
            s.alloc(8)
            raise ValueError
    assert dev.log == ["a1"] and kept.name == "a0"


def test_a_failing_free_does_not_replace_the_exception_in_flight():
    dev = _Dev(failing=("a1",))
    with pytest.raises(KeyError, match="original"):
        with dev.scratch() as s:
            s.alloc(8), s.alloc(8), s.alloc(8)
            raise KeyError("original")
    assert dev.log == ["a2", "a1", "a0"]  # (the buffers after the failing one are freed all the same)


def test_a_failing_free_on_normal_exit_is_raised_after_the_others_are_freed():
    dev = _Dev(failing=("a2", "a0"))
    with pytest.raises(RuntimeError, match="free of a2 failed"):
        with dev.scratch() as s:
            s.alloc(8), s.alloc(8), s.alloc(8)
    assert dev.log == ["a2", "a1", "a0"]


def test_nothing_is_freed_twice():
    dev = _Dev()
    s = dev.scratch()
    with s:
        a = s.alloc(8)
        s.own(_Buf(dev.log, "x"))
        s.keep(a).free()  # (an early free by hand: the scope forgets the buffer first)
    assert dev.log == ["a0", "x"]
    with s:  # (entering the emptied scope again frees nothing more)
        pass
    s.__exit__(None, None, None)
    assert sorted(dev.log) == ["a0", "x"]

