"""Host builds of the headers for the CPU tests: tests/native/<name>.cpp
compiled with g++ into a shared library, loaded with ctypes, every entry's
argument types set from the one table below.  Built once per (name, defines)
and process, into a temporary directory that goes with the process.

    lib = native_build.host_lib("plane_host")
    lib = native_build.host_lib("wide_host", defines=("SDK_PLANE_LC=7",))

SDK_HOST_CFLAGS: extra compiler flags for the default builds of the plane and
canon headers, e.g. SDK_HOST_CFLAGS="-DSDK_PLANE_LC=7" to check a rule-D
variant against its restatement.  A build that names its own defines does not
take them, nor does peer_host (peer_greedy.h has no variants)."""
import ctypes
import os
import subprocess
import tempfile

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
HOST_FLAGS = os.environ.get("SDK_HOST_CFLAGS", "").split()
_NO_HOST_FLAGS = {"peer_host"}

_vp, _i64, _int, _i32, _u32, _u64 = (ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int32, ctypes.c_uint32,
                                     ctypes.c_uint64)
_BATCH = [_vp, _vp, _vp, _i64, _int, _u32]  # in, out, status, n, node_order, max_depth
_CHECK = ([_vp, _i64, _i64, _u64], _i64)    # boards, n, random states, seed -> passes that differ
# library -> entry -> (argtypes, restype)
PROTOS = {
    "plane_host": {
        "plane_solve_batch": (_BATCH + [_u32, _vp, _vp], None),  # mrv_after, guesses, passes
        "plane_check_load": ([_vp, _i64], _i64),
        "plane_check_pass": _CHECK,
        "plane_solve_stats": ([_vp, _i64, _int, _vp, _vp, _vp], None),
        "plane_board_passes": ([_vp, _i64, _int, _vp, _vp], None),
    },
    "wide_host": {
        # mrv_after, lane_guesses, guesses, passes_lane, passes_wide
        "wide_solve_batch": (_BATCH + [_u32, _u32, _vp, _vp, _vp], None),
        "wide_check_fixpoint": ([_vp, _i64, _int, _u32], _i64),
    },
    "ahead_host": {
        "ahead_solve_batch": (_BATCH + [_u32, _int, _vp, _vp], None),  # mrv_after, ahead, guesses, passes
        "ahead_check_pass": _CHECK,
        "ahead_wide_batch": (_BATCH + [_u32, _u32, _vp, _vp], None),  # mrv_after, lane_guesses, passes lane / wide
    },
    "count_host": {
        # in, count, first, n, limit, max_depth, passes, deepest
        "count_host_batch": ([_vp, _vp, _vp, _i64, _i32, _u32, _vp, _vp], None),
    },
    "canon_host": {
        "canon_host_batch": ([_vp, _vp, _vp, _vp, _i64, _int], None),
        "canon_host_slice": ([_vp, _int, _int, _vp], None),
    },
    "peer_host": {
        "peer_host_batch": ([_vp] * 4 + [_i64], None),
        "peer_host_seq": ([_vp] * 4 + [_i64, _vp], None),
    },
}

_dir = None
_libs = {}


def host_lib(name, defines=(), openmp=False):
    """tests/native/<name>.cpp as a loaded ctypes library with its prototypes set."""
    global _dir
    key = (name, tuple(defines))
    if key not in _libs:
        if _dir is None:
            _dir = tempfile.TemporaryDirectory(prefix="sdk_native_")
        out = os.path.join(_dir.name, "lib%s_%d.so" % (name, len(_libs)))
        flags = [] if defines or name in _NO_HOST_FLAGS else HOST_FLAGS
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", *flags, *["-D" + d for d in defines],
                               *(["-fopenmp"] if openmp else []), "-o", out, os.path.join(NATIVE, name + ".cpp")])
        lib = ctypes.CDLL(out)
        for entry, (argtypes, restype) in PROTOS[name].items():
            f = getattr(lib, entry)
            f.argtypes, f.restype = argtypes, restype
        _libs[key] = lib
    return _libs[key]
