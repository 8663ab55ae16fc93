"""rnnl_topk_rows without a GPU: the argument checks (made before any HIP
call) and the numpy restatement the GPU tests compare against."""
import ctypes

import numpy as np
import pytest

import topk_ref


def _call(score, out_index, out_score, out_valid, n_rows=2, n_entities=4, k=2):
    from rnnlogic_amd import _native
    L = _native.lib()
    rc = L.rnnl_topk_rows(score, None, None, None, n_rows, n_entities, k, out_index, out_score, out_valid, None)
    return rc, L.rnnl_last_error()


@pytest.mark.parametrize("bad", ["k0", "k1025", "E0", "rows", "score", "index", "value", "valid"])
def test_argument_validation_without_gpu(bad):
    from rnnlogic_amd import _native
    p = ctypes.c_void_p(64)  # never dereferenced: every case fails the checks
    args = dict(score=p, out_index=p, out_score=p, out_valid=p)
    kw = {}
    if bad == "k0":
        kw["k"] = 0
    elif bad == "k1025":
        kw["k"] = 1025
    elif bad == "E0":
        kw["n_entities"] = 0
    elif bad == "rows":
        kw["n_rows"] = -1
    else:
        args[{"score": "score", "index": "out_index", "value": "out_score", "valid": "out_valid"}[bad]] = None
    rc, msg = _call(args["score"], args["out_index"], args["out_score"], args["out_valid"], **kw)
    assert rc == _native.RNNL_ERR_INVALID
    assert msg == b"rnnl_topk_rows: bad arguments"


def test_no_rows_is_ok_without_launch():
    from rnnlogic_amd import _native
    p = ctypes.c_void_p(64)
    rc, _ = _call(p, p, p, p, n_rows=0, k=_native.TOPK_MAX)
    assert rc == _native.RNNL_OK


def test_reference_agrees_with_sorted():
    nan, inf = float("nan"), float("inf")
    score = np.array([[1.0, 3.0, 3.0, nan, -0.0, 0.0, -inf],
                      [0.0, -0.0, 2.0, 2.0, nan, -inf, 2.0],
                      [-inf, -inf, nan, nan, 5.0, -1.0, -1.0]], dtype=np.float32)
    mask = np.ones((3, 7), dtype=bool)
    mask[1, 2] = False
    flag = np.ones((3, 7), dtype=bool)
    flag[0, 1] = False
    flag[2, 4] = False
    keep = np.array([-1, 3, 4])
    for k in (1, 3, 7, 9):
        index, value, valid = topk_ref.topk_ref(score, mask, flag, keep, k)
        for i in range(3):
            elig = [e for e in range(7) if mask[i, e] and (flag[i, e] or e == keep[i]) and score[i, e] == score[i, e]]
            # Python floats: -0.0 == 0.0, so the sort key ties them and the id decides
            want = sorted(elig, key=lambda e: (-float(score[i, e]), e))[:k]
            assert valid[i] == len(want)
            assert index[i, :len(want)].tolist() == want
            assert (index[i, len(want):] == -1).all() and np.isneginf(value[i, len(want):]).all()
            assert value[i, :len(want)].view(np.uint32).tolist() == score[i, want].view(np.uint32).tolist()
    # the tie, the zeros and the NaN of row 0 at k = 7: 2 (3.0; 1 is flagged out), 0, then -0.0 before +0.0 by id
    assert topk_ref.topk_ref(score, mask, flag, keep, 7)[0][0].tolist() == [2, 0, 4, 5, 6, -1, -1]
