"""What the GPU tests of the one-pass MLE evaluation share: the bindings of
tests/device/mleevalprobe.hip (libtns_mleevalprobe.so) and a restatement of the launch geometry
csrc/mle_eval.hip reports."""
import ctypes as C
import functools
import os

import numpy as np

from oracle import coracle as co

import twist_and_shout as ts
from twist_and_shout import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "multilinear-map-cryptography_amd", "libtns_mleevalprobe.so")
NONE, WAVE, BLOCK, BLOCKS = 0, 1, 2, 3  # MLE_EVAL_* of csrc/ctx.hpp


def plan(nv, batch, min_blocks=256, max_log_rows=6):
    """(regime, launches, blocks of the dot-product launch, rows a thread) as mle_eval.hip decides
    them: one entry a thread up to 2^8 entries an instance -- an instance part of a wave up to 2^6,
    waves of one block above; beyond, 256-entry rows, a thread taking as many rows (a power of two,
    at most 2^max_log_rows and the instance's) as leave the launch min_blocks blocks"""
    if nv <= 8:
        return (WAVE if nv <= 6 else BLOCK, 1, ((batch << nv) + 255) // 256, 1)
    h = nv - 8
    rows, log = batch << h, 0
    while log < min(max_log_rows, 16) and log < h and (rows >> (log + 1)) >= min_blocks:
        log += 1
    return (BLOCK if log == h else BLOCKS, 2, rows >> log, 1 << log)


@functools.lru_cache(maxsize=None)
def lib():
    L = C.CDLL(PROBE)
    L.mleevalprobe_evaluate.restype = C.c_int
    L.mleevalprobe_evaluate.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_uint, C.c_uint64, N.U64P,
                                        C.c_int, C.c_uint64, C.c_int, N.U64P, C.POINTER(C.c_int64)]
    L.mleevalprobe_verify.restype = C.c_int
    L.mleevalprobe_verify.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_uint, C.c_uint64, N.U64P,
                                      C.POINTER(N.TnsTerm), C.c_int, C.POINTER(C.c_void_p), N.U64P, N.U64P, C.c_int,
                                      N.U64P, C.POINTER(C.c_uint32), C.POINTER(C.c_int), N.U64P, C.POINTER(C.c_int64)]
    L.mleevalprobe_fold_chain.restype = C.c_int
    L.mleevalprobe_fold_chain.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_uint, C.c_uint64, N.U64P,
                                          N.U64P]
    assert L.mleevalprobe_info_words() == 4
    return L


def table_ptrs(tabs, bufs):
    """tabs: host arrays (bufs None) or their DeviceBuffers"""
    n = len(tabs)
    return (C.c_void_p * max(1, n))(*([b.ptr for b in bufs] if bufs is not None else [t.ctypes.data for t in tabs]))


def evaluate(tabs, nv, batch, points_mont, bufs=None, min_blocks=0, max_log_rows=-1):
    """the shipped entry point with explicit limits: (status, batch x k x 4 Montgomery values, info =
    regime, launches, blocks, rows a thread); points_mont: batch x nv x 4"""
    k = len(tabs)
    ctx = ts.Context.get(0)
    pts = np.ascontiguousarray(points_mont, dtype=np.uint64).reshape(-1, 4)
    if not len(pts):
        pts = np.zeros((1, 4), dtype=np.uint64)
    out = np.zeros((max(1, batch), max(1, k), 4), dtype=np.uint64)
    info = (C.c_int64 * 4)()
    st = lib().mleevalprobe_evaluate(ctx.handle, table_ptrs(tabs, bufs), k, nv, batch, N.p64(pts), int(bufs is not None),
                                     min_blocks, max_log_rows, N.p64(out), info)
    return st, out[:batch, :k], tuple(info)


def points_array(points):
    """batch rows of nv canonical integers -> batch x nv x 4 Montgomery"""
    batch, nv = len(points), len(points[0]) if points else 0
    flat = [x for p in points for x in p]
    return (co.fr_array(flat) if flat else np.zeros((0, 4), dtype=np.uint64)).reshape(batch, nv, 4)
