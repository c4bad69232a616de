"""tests/native/count_pick_host.cpp for the count-pick tests (host and GPU):
its entries' prototypes, added to native_build's table, and the library per
PICK_VARIANT (0 the header's rule, 1 / 2 the mutants, 3 counting calls, 4 the
rule before)."""
import ctypes

import native_build

_vp, _i64, _int, _u32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_uint32
native_build.PROTOS.setdefault("count_pick_host", {
    "pick_check": ([_i64, ctypes.c_uint64, _vp, _vp], None),  # n, seed, bad[2], seen[6]
    "pick_calls": ([], ctypes.c_uint64),
    # in, out, status, n, node_order, max_depth, mrv_after, ahead, lane_guesses, guesses, passes lane / wide
    "pick_solve_batch": ([_vp, _vp, _vp, _i64, _int, _u32, _u32, _int, _u32, _vp, _vp, _vp], None),
    # in, out, status, n, node_order, max_depth, mrv_after, guesses, passes, passes per board
    "pick_lane_totals": ([_vp, _vp, _vp, _i64, _int, _u32, _u32, _vp, _vp, _vp], None),
})


def lib(variant=0):
    return native_build.host_lib("count_pick_host", ("PICK_VARIANT=%d" % variant,) if variant else ())
