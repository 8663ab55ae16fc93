"""rnnl_miner_paths_side and RuleMiner.explain_paths on the host: the library
exports the call and refuses bad arguments with RNNL_ERR_INVALID and a message
before it touches a device; the Python checks, path_text and the line format of
the predictions file with paths.  Needs no GPU.
"""
import ctypes
import types

import numpy as np
import pytest

from rnnlogic_amd import _native
from rnnlogic_amd import miner as miner_mod


def last_error():
    return _native.lib().rnnl_last_error().decode()


def paths(handle, m=3, c=3, P=3, side=0, n=1):
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(buf)
    return _native.lib().rnnl_miner_paths_side(handle, side, p, n, p, m, p, c, P, p, p, p, p, None)


def test_library_exports_the_call():
    assert hasattr(_native.lib(), "rnnl_miner_paths_side")
    assert "rnnl_miner_paths_side" in [n for n, _, _ in _native.SIGNATURES]
    assert (_native.MINER_PATHS_MAX, _native.MINER_PATH_LEN) == (64, 6)


@pytest.mark.parametrize("kw,word", [(dict(P=0), "max_paths"), (dict(P=65), "max_paths"), (dict(P=-1), "max_paths"),
                                     (dict(m=0), "m ("), (dict(m=257), "m ("), (dict(c=0), "c ("), (dict(c=17), "c ("),
                                     (dict(side=2), "side"), (dict(side=-1), "side"), (dict(), "handle")])
def test_bad_arguments_are_refused_before_the_handle_is_read(kw, word):
    assert paths(None, **kw) == _native.RNNL_ERR_INVALID
    assert "rnnl_miner_paths" in last_error() and word in last_error()


def fake_miner():
    m = object.__new__(miner_mod.RuleMiner)
    m.graph = types.SimpleNamespace(relation_size=2, entity_size=5, id2entity=["ann", "bob", "cy", "dee", "eve"],
                                    id2relation=["likes", "knows"])
    m._rule_off = np.asarray([0, 2, 3], dtype=np.int32)
    m._rule_len = np.asarray([2, 1, 3], dtype=np.int32)
    m._rule_body = np.asarray([[1, 0, 0], [1, 0, 0], [0, 0, 1]], dtype=np.int32)
    m.weights = lambda: [np.asarray([0.5, 0.25]), np.asarray([1.0])]
    return m


def test_python_checks_need_no_device():
    m = fake_miner()
    q, index, rule = [(0, 0, 1)], np.zeros((1, 2), np.int32), np.zeros((1, 2, 3), np.int32)
    for P in (0, 65, -2):
        with pytest.raises(ValueError, match="max_paths must be 1..64"):
            m.explain_paths(q, index, rule, P)
    for bad_rule in (np.zeros((1, 2), np.int32), np.zeros((1, 3, 3), np.int32), np.zeros((2, 2, 3), np.int32),
                     np.zeros((1, 2, 17), np.int32), np.zeros((1, 2, 0), np.int32)):
        with pytest.raises(ValueError, match="rule must be"):
            m.explain_paths(q, index, bad_rule, 3)
    with pytest.raises(ValueError, match="index must be"):
        m.explain_paths(q, np.zeros((2, 2), np.int32), rule, 3)
    with pytest.raises(ValueError, match="side must be"):
        m.explain_paths(q, index, rule, 3, side="both")
    with pytest.raises(ValueError, match="out of range"):
        m.explain_paths([(5, 0, 1)], index, rule, 3)
    with pytest.raises(ValueError, match="2\\^31 elements"):
        m.explain_paths(np.zeros((6000, 3), np.int64), np.zeros((6000, 256), np.int32),
                        np.zeros((6000, 256, 16), np.int32), 64)
    with pytest.raises(ValueError, match="explain > 0"):
        m.predict(triples=q, k=3, explain=0, paths=2)
    with pytest.raises(ValueError, match="paths must be 0..64"):
        m.predict(triples=q, k=3, explain=2, paths=65)


def test_path_text():
    m = fake_miner()
    assert m.path_text([0, 3, 1, -1, -1, -1]) == "ann > dee > bob"
    assert m.path_text(np.asarray([4, 4, -1, -1, -1, -1], dtype=np.int32)) == "eve > eve"
    assert miner_mod.path_text([0, 3, 1, 2, 4, 0]) == "0 > 3 > 1 > 2 > 4 > 0"
    assert m.paths_text(np.asarray([[0, 3, 1, -1, -1, -1], [0, 2, 1, -1, -1, -1]]), 2, 2) == \
        "[ann > dee > bob | ann > cy > bob]"
    assert m.paths_text(np.asarray([[0, 3, 1, -1, -1, -1], [0, 2, 1, -1, -1, -1]]), 2, 7) == \
        "[ann > dee > bob | ann > cy > bob | ...]"
    assert m.paths_text(np.full((2, 6), -1), 0, 0) == "[]"


def hand_made(with_paths):
    out = dict(h=np.asarray([0]), r=np.asarray([0]), t=np.asarray([1]), index=np.asarray([[1, 4]], dtype=np.int32),
               score=np.asarray([[1.5, 0.25]]), valid=np.asarray([2], dtype=np.int32),
               position=np.asarray([0], dtype=np.int32),
               explain_rule=np.asarray([[[0, 1]]], dtype=np.int32), explain_count=np.asarray([[[3, 1]]]))
    if with_paths:
        path = np.full((1, 1, 2, 2, 6), -1, dtype=np.int32)
        path[0, 0, 0, 0, :3], path[0, 0, 0, 1, :3], path[0, 0, 1, 0, :3] = (0, 2, 1), (0, 3, 1), (0, 4, 1)
        out.update(explain_path=path, explain_paths_listed=np.asarray([[[2, 1]]], dtype=np.int32),
                   explain_paths_count=np.asarray([[[3, 1]]], dtype=np.int64))
    return out


def test_prediction_lines_with_and_without_paths(tmp_path):
    m = fake_miner()
    m._write_predictions(str(tmp_path / "plain.tsv"), hand_made(False), 1)
    m._write_predictions(str(tmp_path / "paths.tsv"), hand_made(True), 1)
    plain = (tmp_path / "plain.tsv").read_text().splitlines()
    assert plain == ["ann\tlikes\t1\tbob\t1.5\t*\tlikes <- knows, likes:3:0.5\tlikes <- knows:1:0.25",
                     "ann\tlikes\t2\teve\t0.25\t"]
    assert (tmp_path / "paths.tsv").read_text().splitlines() == [
        "ann\tlikes\t1\tbob\t1.5\t*\tlikes <- knows, likes:3:0.5 [ann > cy > bob | ann > dee > bob | ...]"
        "\tlikes <- knows:1:0.25 [ann > eve > bob]",
        "ann\tlikes\t2\teve\t0.25\t"]
