"""runtime.capture_gc (CPU): the guard GraphRunner puts around its stream capture.  A dead reference cycle is freed
before the block runs, the automatic collector stays off inside it, and its earlier state comes back afterwards, also
when the block raises."""
import gc
import weakref

import pytest

import s2v_import  # noqa: F401
from s2v_amd import runtime


class Node:
    pass


def dead_cycle():
    a, b = Node(), Node()
    a.other, b.other = b, a
    return weakref.ref(a)


def test_collects_first_and_keeps_the_collector_off():
    assert gc.isenabled()
    gc.disable()                                              # so that only capture_gc can free the cycle
    try:
        ref = dead_cycle()
        assert ref() is not None
        gc.enable()
        with runtime.capture_gc():
            assert ref() is None and not gc.isenabled()
            inner = dead_cycle()
            for _ in range(5000):                             # far past the generation-0 threshold
                Node().other = Node()
            assert inner() is not None
        assert gc.isenabled()
    finally:
        gc.enable()


def test_restores_the_state_it_found():
    gc.disable()
    try:
        with runtime.capture_gc():
            assert not gc.isenabled()
        assert not gc.isenabled()                             # it was off before: it stays off
    finally:
        gc.enable()
    with pytest.raises(RuntimeError):
        with runtime.capture_gc():
            raise RuntimeError("capture failed")
    assert gc.isenabled()


def test_graph_runner_captures_inside_the_guard():
    import inspect
    src = inspect.getsource(runtime.GraphRunner.__init__)
    assert "with capture_gc(), torch.cuda.graph(self.graph):" in src
