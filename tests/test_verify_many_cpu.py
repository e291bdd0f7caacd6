"""The sound batched KZG verifier's host side (tns_verify_challenges; kzg_verify.hip's entry points
refusing NULL handles before they touch a device, in the manner of test_vector_open_all_cpu.py).
Runs without a GPU."""
import ctypes as C
import struct

import numpy as np
import pytest

from oracle import pyoracle as po

import twist_and_shout as ts
from twist_and_shout import _native as N

SEEDS = [bytes([42] * 32), bytes(range(1, 33))]


def reference_challenges(seed, upto):
    """gamma_i = the i-th u128 of ChaCha20Rng::from_seed(seed): next_u64() | next_u64() << 64."""
    rng = po.ChaCha20Rng(seed)
    out = []
    for _ in range(upto):
        lo = rng.next_u64()
        out.append(lo | rng.next_u64() << 64)
    return out


@pytest.mark.parametrize("seed", SEEDS)
def test_challenges_are_the_chacha20_word_stream(seed):
    want = reference_challenges(seed, 80)
    assert all(0 < g < 1 << 128 for g in want)  # (no zero among them: the 0 -> 1 rule is not in play)
    # 3 | 4: the four-per-block boundary; 63 | 64 | 65: the reference generator's 64-word buffer
    # holds challenges 0..15, so 15 | 16 is its refill and 63 | 64 the fourth one
    for first, count in [(0, 9), (3, 2), (4, 5), (15, 2), (63, 1), (63, 3), (64, 4), (65, 7)]:
        assert ts.verify_challenges(seed, first, count) == want[first:first + count], (first, count)
    assert ts.verify_challenges(seed, 5, 0) == []


def test_challenges_far_into_the_stream():
    # position 2^34 + 1: block counter 2^32 -- the counter's high word is in use
    seed = SEEDS[1]
    first = (1 << 34) + 1
    blk = po.chacha20_block(list(struct.unpack("<8I", seed)), first // 4)
    w = blk[4 * (first % 4):4 * (first % 4) + 4]
    assert ts.verify_challenges(seed, first, 1) == [w[0] | w[1] << 32 | w[2] << 64 | w[3] << 96]


def test_entry_points_refuse_null_before_any_device():
    lib = N.load()
    vk = N.TnsVk()
    pts = np.zeros((2, 8), dtype=np.uint64)
    fr = np.zeros((2, 4), dtype=np.uint64)
    proj = np.zeros(12, dtype=np.uint64)
    seed = (C.c_uint8 * 32)(*SEEDS[0])
    ok = C.c_int(-7)
    bad = C.c_uint64(77)
    okp, badp = C.byref(ok), C.pointer(bad)
    assert lib.tns_kzg_verify_many(None, C.byref(vk), N.p64(pts), 2, N.p64(fr), N.p64(fr), N.p64(pts), 2, seed,
                                   okp, badp) == 1
    assert lib.tns_kzg_verify_many(None, None, None, 0, None, None, None, 0, None, None, None) == 1
    assert lib.tns_vc_verify_all(None, C.byref(vk), N.p64(proj), N.p64(fr), 2, N.p64(pts), seed, okp, badp) == 1
    assert lib.tns_vc_verify_all(None, None, None, None, 2, None, None, None, None) == 1
    assert lib.tns_vc_verify_all_device(None, C.byref(vk), N.p64(proj), None, 2, None, seed, okp, badp) == 1
    assert b"null" in lib.tns_last_error()
    assert ok.value == -7 and bad.value == 77
