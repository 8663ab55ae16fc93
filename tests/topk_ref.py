"""numpy restatement of rnnl_topk_rows (include/rnnlogic_hip.h): per row the
first k eligible entities by score descending, then entity id ascending.

Eligible: mask (if given) set, flag (if given) set or the entity is the row's
`keep`, and the score is not NaN.  `-(score + 0.0)` folds -0.0 onto +0.0 and a
stable argsort over the ascending eligible ids breaks ties by id.  Unused slots
are -1 / -inf; valid = min(k, #eligible).
"""
import numpy as np


def topk_ref(score, mask=None, flag=None, keep=None, k=1):
    score = np.asarray(score, dtype=np.float32)
    n, E = score.shape
    index = np.full((n, k), -1, dtype=np.int32)
    value = np.full((n, k), -np.inf, dtype=np.float32)
    valid = np.zeros(n, dtype=np.int32)
    for i in range(n):
        ok = ~np.isnan(score[i])
        if mask is not None:
            ok &= np.asarray(mask[i]) != 0
        if flag is not None:
            f = np.asarray(flag[i]) != 0
            if keep is not None and 0 <= int(keep[i]) < E:
                f = f.copy()
                f[int(keep[i])] = True
            ok &= f
        ids = np.nonzero(ok)[0]
        order = np.argsort(-(score[i, ids] + np.float32(0.0)), kind="stable")
        top = ids[order][:k]
        valid[i] = len(top)
        index[i, :len(top)] = top
        value[i, :len(top)] = score[i, top]
    return index, value, valid


def assert_equal(got, want, what=""):
    """Exact comparison of (index, score, valid): score bit for bit."""
    gi, gs, gv = [np.asarray(x) for x in got]
    wi, ws, wv = want
    np.testing.assert_array_equal(gv, wv, err_msg="%s valid" % what)
    np.testing.assert_array_equal(gi, wi, err_msg="%s index" % what)
    np.testing.assert_array_equal(gs.view(np.uint32), ws.view(np.uint32), err_msg="%s score bits" % what)
