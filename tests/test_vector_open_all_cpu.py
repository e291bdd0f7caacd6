"""The all-index vector-commitment entry points (tns_vc_open_all, tns_vc_open_all_device,
tns_srs_prepare_open_all, tns_vc_open_many) refuse NULL handles before touching a device, in the
manner of test_abi.py::test_null_arguments_are_invalid_parameters.  Runs without a GPU."""
import numpy as np

from twist_and_shout import _native as N


def test_open_all_entry_points_refuse_null():
    lib = N.load()
    vec = np.zeros((2, 4), dtype=np.uint64)
    idx = np.zeros(2, dtype=np.uint64)
    out = np.full((2, 12), 7, dtype=np.uint64)
    assert lib.tns_vc_open_all(None, None, N.p64(vec), 2, N.p64(out)) == 1
    assert lib.tns_vc_open_all(None, None, None, 2, None) == 1
    assert lib.tns_vc_open_all_device(None, None, None, 2, None) == 1
    assert lib.tns_srs_prepare_open_all(None, None, 2) == 1
    assert lib.tns_vc_open_many(None, None, N.p64(vec), 2, N.p64(idx), 2, N.p64(out), N.p64(out)) == 1
    assert lib.tns_vc_open_many(None, None, None, 2, None, 0, None, None) == 1
    assert b"null" in lib.tns_last_error()
    assert (out == 7).all()
