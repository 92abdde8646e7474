"""Strided bond history, host side (no GPU): the C-ABI surface of
yuma_run_opts / yuma_graph_create_opts / yuma_hist_slots and the slot
arithmetic of engine.hist_epochs against a plain Python range."""

from __future__ import annotations

import ctypes
import os
import re

import pytest

from yuma_simulation._internal import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("yuma_run_opts", "yuma_graph_create_opts", "yuma_hist_slots")

ES = (1, 4, 11, 12)
STRIDES = (1, 2, 3, 5, 11, 12, 40)


def firsts(E):
    return (None, 0, 2, E - 1, E, E + 3)


def header_text():
    text = open(os.path.join(ROOT, "include", "yuma_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_options_record_and_entry_points():
    text = header_text()
    m = re.search(r"typedef\s+struct\s+yuma_run_options\s*\{(.*?)\}\s*yuma_run_options_t\s*;", text, flags=re.S)
    assert m, "yuma_run_options / yuma_run_options_t not declared"
    fields = re.findall(r"int32_t\s+(\w+)(?:\[(\d+)\])?\s*;", m.group(1))
    assert fields == [("flags", ""), ("hist_stride", ""), ("hist_first", ""), ("reserved", "5")]
    for name in NEW_FUNCTIONS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
    # the entry points take the record by pointer, in place of the flags word
    for name in ("yuma_run_opts", "yuma_graph_create_opts"):
        proto = re.search(name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert "const yuma_run_options_t* opts" in proto and "int flags" not in proto, name


def test_library_exports_the_entry_points():
    lib = engine.load_library()
    for name in NEW_FUNCTIONS:
        assert name in engine.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert ctypes.sizeof(engine.YumaRunOptionsC) == 32
    # yuma_run_opts is yuma_run_ex with the record in place of `int flags`
    ex, op = lib.yuma_run_ex.argtypes, lib.yuma_run_opts.argtypes
    assert len(ex) == len(op)
    assert [a for a, b in zip(ex, op) if a is not b] == [ctypes.c_int]
    assert len(lib.yuma_graph_create_opts.argtypes) == len(lib.yuma_graph_create_ex.argtypes)


@pytest.mark.parametrize("E", ES)
def test_hist_epochs_is_the_plain_range(E):
    lib = engine.load_library()
    empty = 0
    for stride in STRIDES:
        for first in firsts(E):
            f = stride - 1 if first is None else first
            expected = tuple(t for t in range(E) if t >= f and (t - f) % stride == 0)
            got = engine.hist_epochs(E, stride, first)
            assert isinstance(got, tuple) and got == expected, (E, stride, first)
            assert lib.yuma_hist_slots(E, stride, f) == len(expected), (E, stride, first)
            # the issue's closed form
            assert len(expected) == ((E - 1 - f) // stride + 1 if f < E else 0)
            if f >= E:
                assert got == ()
                empty += 1
    assert empty >= 2 * len(STRIDES)  # first = E and E + 3 at every stride
    assert engine.hist_epochs(E) == tuple(range(E))  # the dense history
    assert lib.yuma_hist_slots(E, 0, 0) == E  # stride 0 counts as 1


def test_bad_arguments_are_refused():
    lib = engine.load_library()
    for kw in (dict(stride=0), dict(stride=-3), dict(first=-1), dict(stride=2, first=-5)):
        with pytest.raises(ValueError):
            engine.hist_epochs(11, **kw)
    for args in ((11, -1, 0), (11, 3, -1), (0, 1, 0), (-4, 1, 0)):
        assert lib.yuma_hist_slots(*args) < 0, args
        assert lib.yuma_last_error()  # a text goes with the code


@pytest.mark.parametrize("bad", [dict(hist_stride=-1), dict(hist_first=-1), dict(flags=1 << 10),
                                 dict(reserved=(0, 0, 1, 0, 0)), dict(reserved=(0, 0, 0, 0, -1))])
def test_bad_options_return_einval_before_any_launch(bad):
    """The options are checked first: the rest of the call is never looked at
    (null pointers here), so this runs without a GPU."""
    lib = engine.load_library()
    opts = engine.YumaRunOptionsC(**bad)
    run_args = (3, None, 1, 11, 8, 64, None, None, None, None, None, None, 0, 0)
    assert lib.yuma_run_opts(*run_args, ctypes.addressof(opts), None, None) == -1
    text = lib.yuma_last_error().decode()
    assert any(w in text for w in ("hist_stride", "reserved", "flags")), text
    h = ctypes.c_void_p()
    assert lib.yuma_graph_create_opts(ctypes.byref(h), *run_args, ctypes.addressof(opts)) == -1
    assert not h.value


def test_run_result_keeps_its_positional_fields():
    """hist_epochs trails with a default: six-field constructions still work."""
    r = engine.RunResult(None, None, None, None, None, {})
    assert r.hist_epochs is None
