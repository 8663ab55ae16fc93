"""The head side of the miner on the host: read_queries_file(side="head"), the
command line's -side checks that come before a miner exists, the three
rnnl_miner_*_side entry points refusing an unknown side before any device
call, and the Python argument errors that need no device.  Needs no GPU.
"""
import ctypes
import types

import numpy as np
import pytest

from rnnlogic_amd import _native
from rnnlogic_amd import miner as miner_mod


def toy_graph():
    return types.SimpleNamespace(entity2id={"ann": 0, "bob": 1, "cy d": 2}, relation2id={"likes": 0, "knows": 1},
                                 entity_size=3, relation_size=2)


def test_read_queries_file_on_the_head_side(tmp_path):
    f = tmp_path / "q.tsv"
    f.write_text("\tlikes\tbob\nann\tknows\tcy d\n\n\tknows\tann\r\n")
    got = miner_mod.read_queries_file(str(f), toy_graph(), side="head")
    assert got.dtype == np.int64 and got.tolist() == [[-1, 0, 1], [0, 1, 2], [-1, 1, 0]]
    # the tail side reads what it read before, with and without the argument
    f.write_text("ann\tlikes\nann\tknows\tcy d\n")
    want = [[0, 0, -1], [0, 1, 2]]
    assert miner_mod.read_queries_file(str(f), toy_graph()).tolist() == want
    assert miner_mod.read_queries_file(str(f), toy_graph(), "tail").tolist() == want
    with pytest.raises(ValueError, match=r"q\.tsv:1"):  # two fields: (h, r) is no head query
        miner_mod.read_queries_file(str(f), toy_graph(), side="head")
    for text, where in (("\tlikes\tbob\nann\tlikes\n", "q.tsv:2"), ("\tlikes\tbob\tann\n", "q.tsv:1"),
                        ("\tlikes\tzed\n", "zed"), ("zed\tlikes\tbob\n", "zed"), ("\tloves\tbob\n", "loves"),
                        ("ann\tlikes\t\n", "q.tsv:1"), ("\t\tbob\n", "q.tsv:1")):
        f.write_text(text)
        with pytest.raises(ValueError) as err:
            miner_mod.read_queries_file(str(f), toy_graph(), side="head")
        assert where in str(err.value)
    with pytest.raises(ValueError, match="side"):
        miner_mod.read_queries_file(str(f), toy_graph(), side="both")


@pytest.mark.parametrize("how", [["-predict", "test"], ["-queries-file", "q.tsv"]])
def test_side_both_with_predictions_is_refused_before_a_miner_exists(how, monkeypatch, capsys):
    def no_miner(*a, **k):
        raise AssertionError("the miner was created")
    monkeypatch.setattr(miner_mod, "RuleMiner", no_miner)
    with pytest.raises(SystemExit) as err:
        miner_mod.main(["-data-path", "/nonexistent", "-rule-file", "rules.txt", "-predictions-file", "p.tsv", "-side",
                        "both"] + how)
    assert err.value.code == 2 and "-side both" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        miner_mod.main(["-data-path", "/nonexistent", "-rule-file", "rules.txt", "-evaluate", "test", "-side", "up"])
    assert "-side" in capsys.readouterr().err


def bare_miner():
    """A RuleMiner without a device handle: argument checks come before any device call."""
    m = object.__new__(miner_mod.RuleMiner)
    m.graph = types.SimpleNamespace(relation_size=2, entity_size=5)
    return m


def test_head_side_query_shapes_and_ranges():
    m = bare_miner()
    assert m._pred_queries([(-1, 1, 4), (4, 0, 0)], "head").tolist() == [[-1, 1, 4], [4, 0, 0]]
    assert m._pred_queries([], "head").shape == (0, 3)
    for bad in ([(0, 1)], [(0, 1, -1)], [(-2, 1, 0)], [(5, 1, 0)], [(0, 2, 0)], [(0, 1, 5)], [(0, -1, 0)]):
        with pytest.raises(ValueError):
            m._pred_queries(bad, "head")
    assert m._pred_queries([(0, 1)], "tail").tolist() == [[0, 1, -1]]  # (h, r) stays the tail side's open form
    for call in (lambda: m.predict_topk([(0, 1, 2)], side="left"), lambda: m.explain([(0, 1, 2)], [[1]], side="both"),
                 lambda: m.scores([(0, 1, 2)], side="both"), lambda: m.eval_ranks([(0, 1, 2)], side="heads"),
                 lambda: m.evaluate(triples=[(0, 1, 2)], side="all"),
                 lambda: m.predict(triples=[(0, 1, 2)], side="both")):
        with pytest.raises(ValueError, match="side"):
            call()


def test_library_exports_the_side_calls_and_refuses_an_unknown_side():
    L = _native.lib()
    names = [n for n, _, _ in _native.SIGNATURES]
    for name in ("rnnl_miner_evaluate_side", "rnnl_miner_predict_side", "rnnl_miner_explain_side"):
        assert hasattr(L, name) and name in names
    assert (_native.MINER_TAIL, _native.MINER_HEAD) == (0, 1)
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(buf)
    for side in (2, -1, 1 << 20):  # decided before the handle is looked at
        assert L.rnnl_miner_evaluate_side(None, side, p, 1, None, None, None, 0, p, None, p, None) == \
            _native.RNNL_ERR_INVALID
        assert "rnnl_miner_evaluate_side" in L.rnnl_last_error().decode() and "side" in L.rnnl_last_error().decode()
        assert L.rnnl_miner_predict_side(None, side, p, 1, None, None, None, 0, 10, 0, p, p, p, p, p, None) == \
            _native.RNNL_ERR_INVALID
        assert "rnnl_miner_predict_side" in L.rnnl_last_error().decode()
        assert L.rnnl_miner_explain_side(None, side, p, 1, p, 3, 3, p, p, p, p, p, None) == _native.RNNL_ERR_INVALID
        assert "rnnl_miner_explain_side" in L.rnnl_last_error().decode()
    for side in (_native.MINER_TAIL, _native.MINER_HEAD):  # a known side goes on to the other checks
        assert L.rnnl_miner_predict_side(None, side, p, 1, None, None, None, 0, 10, 0, p, p, p, p, p, None) == \
            _native.RNNL_ERR_INVALID
        assert "handle" in L.rnnl_last_error().decode()
        assert L.rnnl_miner_evaluate_side(None, side, p, 1, None, None, None, 0, p, None, p, None) == \
            _native.RNNL_ERR_INVALID
        assert "bad arguments" in L.rnnl_last_error().decode()
