"""rnnl_miner_predict / rnnl_miner_explain on the host: the library exports
them and refuses bad arguments with RNNL_ERR_INVALID and a message before it
touches a device.  Needs no GPU.
"""
import ctypes

import pytest

from rnnlogic_amd import _native


def last_error():
    return _native.lib().rnnl_last_error().decode()


def predict(handle, k, candidates=0, known=(None, None, None)):
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(buf)
    return _native.lib().rnnl_miner_predict(handle, p, 1, known[0], known[1], known[2], 0, k, candidates, p, p, p, p,
                                            p, None)


def explain(handle, m, c):
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(buf)
    return _native.lib().rnnl_miner_explain(handle, p, 1, p, m, c, p, p, p, p, p, None)


def test_library_exports_both_calls():
    L = _native.lib()
    assert hasattr(L, "rnnl_miner_predict") and hasattr(L, "rnnl_miner_explain")
    names = [n for n, _, _ in _native.SIGNATURES]
    assert "rnnl_miner_predict" in names and "rnnl_miner_explain" in names
    assert (_native.MINER_TOPK_MAX, _native.MINER_EXPLAIN_MAX) == (256, 16)


def test_null_handle_is_refused():
    assert predict(None, 10) == _native.RNNL_ERR_INVALID
    assert "rnnl_miner_predict" in last_error() and "handle" in last_error()
    assert explain(None, 3, 3) == _native.RNNL_ERR_INVALID
    assert "rnnl_miner_explain" in last_error() and "handle" in last_error()


@pytest.mark.parametrize("k", [0, -1, 257, 1 << 20])
def test_k_out_of_range(k):
    assert predict(None, k) == _native.RNNL_ERR_INVALID
    assert "k must be 1..256" in last_error()


def test_candidates_and_partial_known_arrays():
    assert predict(None, 10, candidates=2) == _native.RNNL_ERR_INVALID
    assert "candidates" in last_error()
    buf = (ctypes.c_int64 * 2)()
    assert predict(None, 10, known=(ctypes.addressof(buf), None, None)) == _native.RNNL_ERR_INVALID
    assert "all or none" in last_error()


@pytest.mark.parametrize("m,c,word", [(0, 3, "m ("), (257, 3, "m ("), (3, 0, "c ("), (3, 17, "c ("), (-1, 1, "m (")])
def test_slots_and_rules_per_slot_out_of_range(m, c, word):
    assert explain(None, m, c) == _native.RNNL_ERR_INVALID
    assert "rnnl_miner_explain" in last_error() and word in last_error()
