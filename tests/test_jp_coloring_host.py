"""The specification of the device colouring (gmg_config::device_coloring): csrc/host_plan.hpp::jp_coloring_host through gmg_jp_coloring_host --
Jones-Plassmann in synchronous rounds, priority (mix32(v), v), first-fit colours.  No device needed.  Every case asks for a proper colouring with
the colours 0 .. n_colors - 1, for the bytes and the round count of the numpy restatement in tests/jp_coloring_cases.py, for the same bytes
from other representations of the pattern, and for at most (maximum degree + 1) colours -- which first fit guarantees: a winner has at most
deg coloured neighbours, so one of the colours 0 .. deg is free."""
import ctypes as C

import numpy as np
import pytest

from tests import jp_coloring_cases as cases


@pytest.mark.parametrize("name", list(cases.cases()))
def test_host_colouring_is_the_specification(cabi, name):
    indptr, indices = cases.cases()[name]
    colours, ncol, rounds = cabi.jp_coloring(indptr, indices)
    n = len(indptr) - 1
    assert colours is not None and colours.shape == (n,) and ncol >= 1 and rounds >= 1
    cases.assert_proper(indptr, indices, colours, ncol)
    want, want_ncol, want_rounds = cases.restatement(indptr, indices)
    assert (ncol, rounds) == (want_ncol, want_rounds)
    assert np.array_equal(colours, want)
    assert ncol <= int(cases.degrees(indptr, indices).max(initial=0)) + 1
    for ptr2, idx2 in cases.other_representations(indptr, indices):
        c2, n2, r2 = cabi.jp_coloring(ptr2, idx2)
        assert (n2, r2) == (ncol, rounds) and np.array_equal(c2, colours)


def test_complete_graph_of_70_takes_70_colours(cabi):
    colours, ncol, rounds = cabi.jp_coloring(*cases.cases()["complete70"])
    assert ncol == 70 and rounds == 70 and sorted(colours) == list(range(70))       # one winner per round; colours 64 .. 69 from the general path


def test_isolated_vertices_and_loops(cabi):
    colours, ncol, rounds = cabi.jp_coloring(*cases.cases()["isolated-and-loop"])
    assert colours[4] == 0 and colours[5] == 0 and ncol == 2
    assert cabi.jp_coloring(*cases.cases()["single"]) [1:] == (1, 1)
    c, ncol, rounds = cabi.jp_coloring(np.array([0, 0], np.int32), np.zeros(0, np.int32))       # n = 1 without any entry
    assert c.tolist() == [0] and (ncol, rounds) == (1, 1)


def test_more_than_254_colours_is_minus_one(cabi):
    indptr, indices = cases.complete(300)
    colours, ncol, rounds = cabi.jp_coloring(indptr, indices)
    assert colours is None and ncol == -1 and rounds == 0
    assert cases.restatement(indptr, indices)[1] == -1
    # 254 vertices still fit: colours 0 .. 253
    colours, ncol, _ = cabi.jp_coloring(*cases.complete(254))
    assert ncol == 254 and sorted(colours) == list(range(254))
    assert cabi.jp_coloring(*cases.complete(255))[1] == -1


def test_arrays_that_would_take_a_reader_out_of_bounds_are_refused(cabi):
    out = (C.c_ubyte * 4)()
    ncol, rounds = C.c_int(0), C.c_int(0)
    def call(ptr, idx):
        ptr = np.asarray(ptr, np.int32); idx = np.asarray(idx, np.int32)
        return cabi.lib().gmg_jp_coloring_host(len(ptr) - 1, cabi._pi(ptr), cabi._pi(idx), out, C.byref(ncol), C.byref(rounds))
    assert call([0, 1, 2], [1, 0]) == 0
    assert call([0, 1, 2], [1, 2]) == cabi.GMG_ERR_INVALID          # index past n - 1
    assert call([0, 1, 2], [-1, 0]) == cabi.GMG_ERR_INVALID
    assert call([0, 2, 1], [1, 0]) == cabi.GMG_ERR_INVALID          # pointers decrease
    assert call([1, 1, 2], [1, 0]) == cabi.GMG_ERR_INVALID          # pointers do not start at 0


def test_config_mirror_has_the_option_in_front_of_accelerate(cabi):
    names = [f[0] for f in cabi.GmgConfig._fields_]
    assert names[-2:] == ["device_coloring", "accelerate"]
    assert cabi.lib().gmg_config_size() == C.sizeof(cabi.GmgConfig)
    cfg = cabi.GmgConfig()
    assert cabi.lib().gmg_config_default(C.byref(cfg)) == 0 and cfg.device_coloring == 0
    for bad in (2, -1):
        with pytest.raises(cabi.GmgError) as e:
            cabi.Engine(device_coloring=bad)
        assert e.value.code == cabi.GMG_ERR_INVALID
