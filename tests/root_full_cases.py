"""Shared pieces of the root-rule tests (test_root_full.py on the CPU,
test_gpu_root_full.py on the GPU): the host entry of tests/native/
rootfull_host.cpp and the fixture tests/golden/root_full_cases.json, boards
whose root propagation ends all single and is no completion
(tests/golden/make_root_full_cases.py finds them)."""
import ctypes
import functools
import json
import os

import numpy as np

import native_build

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "root_full_cases.json")

_vp, _i64, _int, _u32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_uint32
native_build.PROTOS.setdefault("rootfull_host", {
    # in, n, node_order, max_depth, mrv_after, out/status without and with the
    # rule, passes without / with, ended by the rule, rejected
    "rootfull_compare": ([_vp, _i64, _int, _u32, _u32] + [_vp] * 8, None),
    # in, out, status, n, node_order, max_depth, mrv_after, root_full
    "rootfull_solve_ahead": ([_vp, _vp, _vp, _i64, _int, _u32, _u32, _int], None),
    "rootfull_grid_complete": ([_vp, _i64, _vp], None),
})


def lib():
    return native_build.host_lib("rootfull_host")


def compare(boards, node_order=0, mrv_after=128, max_depth=32):
    """Both runs of rootfull_compare on `boards`, as a dict of arrays:
    out_off / st_off / out_on / st_on, passes_off / passes_on, by_rule,
    rejected."""
    boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
    n = len(boards)
    r = {"out_off": np.zeros_like(boards), "st_off": np.zeros(n, np.int32), "out_on": np.zeros_like(boards),
         "st_on": np.zeros(n, np.int32), "passes_off": np.zeros(n, np.uint32), "passes_on": np.zeros(n, np.uint32),
         "by_rule": np.zeros(n, np.uint8), "rejected": np.zeros(n, np.uint8)}
    lib().rootfull_compare(boards.ctypes.data, n, node_order, max_depth, mrv_after, *[a.ctypes.data for a in r.values()])
    return r


def grid_complete(grids):
    grids = np.ascontiguousarray(grids, dtype=np.uint8).reshape(-1, 81)
    ok = np.zeros(len(grids), np.uint8)
    lib().rootfull_grid_complete(grids.ctypes.data, len(grids), ok.ctypes.data)
    return ok.astype(bool)


@functools.lru_cache(maxsize=None)
def load_fixture():
    """(k, 81) uint8 boards (read-only): clean givens, no completion, an
    all-single root after propagation."""
    with open(FIXTURE) as f:
        doc = json.load(f)
    boards = np.array([[int(c) for c in case["board"]] for case in doc["cases"]], dtype=np.uint8)
    assert all(case["count"] == 0 for case in doc["cases"])
    boards.setflags(write=False)
    return boards
