"""The miner's aggregations on the host: the pure functions behind
RuleMiner.set_aggregation (noisy_or_operand, max_classes, decode_max,
noisy_or_probability), the command line's checks that come before a miner
exists, and rnnl_miner_set_aggregation refusing an unknown mode or depth before
it looks at the handle.  Needs no GPU.
"""
import math
import types

import numpy as np
import pytest

import mine_agg_ref as A
from rnnlogic_amd import _native
from rnnlogic_amd import miner as miner_mod


def test_noisy_or_operand_is_log1p_per_element():
    rng = np.random.default_rng(3)
    ws = [rng.random(500).tolist() + [0.0, 1.0, 0.5, 2.0 ** -60, 1.0 - 2.0 ** -53], [], [0.25]]
    got = miner_mod.noisy_or_operand(ws)
    assert [len(g) for g in got] == [505, 0, 1] and all(g.dtype == np.float64 for g in got)
    for g, w in zip(got, ws):
        assert g.tolist() == [-math.log1p(-min(x, 1.0 - 2.0 ** -53)) for x in w]
        assert g.tolist() == [A.noisy_or_u(x) for x in w]  # the restatement's own
    # the clamp: w = 1 is the largest double below 1, -log(2^-53), not inf
    assert got[0][501] == got[0][504] == 53 * math.log(2.0) and np.isfinite(got[0]).all()
    assert got[0][500] == 0.0 and not np.signbit(got[0][500])
    # the probability for display inverts it
    assert np.allclose(miner_mod.noisy_or_probability(got[0][:500]), ws[0][:500], rtol=0, atol=1e-15)
    assert miner_mod.noisy_or_probability(0.0) == 0.0
    assert miner_mod.noisy_or_probability(np.asarray([got[0][1] + got[0][2]]))[0] == \
        -math.expm1(-(got[0][1] + got[0][2]))


def test_max_classes_with_repeated_and_zero_weights():
    classes, values = miner_mod.max_classes([[1.0, .5, .5, .25, 0, .5, .125, .75, 1.0], [], [0.0, 0.0], [7.5]])
    assert classes[0].tolist() == [5, 3, 3, 2, 0, 3, 1, 4, 5] and values[0].tolist() == [.125, .25, .5, .75, 1.0]
    assert classes[1].tolist() == [] and values[1].tolist() == []
    assert classes[2].tolist() == [0, 0] and values[2].tolist() == []
    assert classes[3].tolist() == [1] and values[3].tolist() == [7.5]  # max takes any finite weight >= 0
    for ws in ([[1.0, .5, .5, .25, 0, .5]], A.TINY_WEIGHTS):
        got = miner_mod.max_classes(ws)
        assert [c.tolist() for c in got[0]] == [A.classes_of(w)[0] for w in ws]
        assert [v.tolist() for v in got[1]] == [A.classes_of(w)[1] for w in ws]


def test_class_count_boundary():
    w = np.arange(1, miner_mod.MAX_CLASSES + 1, dtype=np.float64)
    assert miner_mod.MAX_CLASSES == 131071 == _native.MINER_AGG_CLASS_MAX
    classes, values = miner_mod.max_classes([[], np.concatenate([w, w[:5], [0.0]])])
    assert classes[1].max() == 131071 and classes[1][-1] == 0 and len(values[1]) == 131071
    with pytest.raises(ValueError, match=r"relation 1 .*131072 distinct"):
        miner_mod.max_classes([[], np.arange(1, 131073, dtype=np.float64)])


def test_decode_max_inverts_the_key():
    values = np.asarray([.125, .25, .5, .75, 1.0])
    keys = [A.max_key(cs, d) for cs, d in (([5, 3, 3], 3), ([5, 3, 3], 2), ([5, 3, 3], 1), ([2], 3), ([], 3),
                                           ([1, 1, 1, 1], 3), ([0, 4, 0], 3))]
    got = miner_mod.decode_max(keys, values)
    assert got.shape == (7, 3)
    assert got.tolist() == [[1.0, .5, .5], [1.0, .5, 0.0], [1.0, 0.0, 0.0], [.25, 0.0, 0.0], [0.0, 0.0, 0.0],
                            [.125, .125, .125], [.75, 0.0, 0.0]]
    assert miner_mod.decode_max(np.asarray(keys).reshape(7, 1), values).shape == (7, 1, 3)
    # the largest key is exact in a double
    top = A.max_key([131071, 131071, 131071], 3)
    assert top == float(2 ** 51 - 1) and int(top) == 2 ** 51 - 1
    big = np.arange(1, 131072, dtype=np.float64)
    assert miner_mod.decode_max(top, big).tolist() == [131071.0] * 3
    for bad in (-1.0, 0.5, float("nan"), float(2 ** 51), A.max_key([6], 1)):
        with pytest.raises(ValueError, match="decode_max"):
            miner_mod.decode_max(bad, values)


def test_weights_a_mode_does_not_admit():
    for bad in (1.5, -0.25, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"noisy_or: .*rule 2 of relation 1 "):
            miner_mod.noisy_or_operand([[0.5], [0.0, 1.0, bad, 3.0]])
    for bad in (-0.25, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"max: .*rule 1 of relation 2 "):
            miner_mod.max_classes([[], [2.5], [0.5, bad]])
    miner_mod.max_classes([[1.5, 1e300]])  # finite and >= 0 is all max asks


def bare_miner():
    m = object.__new__(miner_mod.RuleMiner)
    m.graph = types.SimpleNamespace(relation_size=2, entity_size=5)
    return m


def test_set_aggregation_arguments_and_display_values():
    m = bare_miner()
    assert m.aggregation == ("sum", 1)
    for agg, depth in (("mean", 1), ("max", 0), ("max", 4), ("noisy_or", 2.5), (None, 1)):
        with pytest.raises(ValueError, match="set_aggregation"):
            m.set_aggregation(agg, depth)
    assert m.aggregation == ("sum", 1)
    s = np.asarray([[0.0, 1.5, -np.inf]])
    assert m.score_value(s, 0) is not None and np.array_equal(m.score_value(s, 0), s)  # sum: the score itself
    m.set_aggregation("max", 2)
    assert m.aggregation == ("max", 2)
    m.set_aggregation("noisy-or")  # the command line's spelling
    assert m.aggregation == ("noisy_or", 1)
    assert m.score_value(s, 0).tolist() == [[0.0, -math.expm1(-1.5), -np.inf]]
    m.set_aggregation("sum", 3)
    assert m.aggregation == ("sum", 1)


@pytest.mark.parametrize("args, word", [
    (["-agg", "mean"], "-agg"),
    (["-agg", "max", "-agg-depth", "4"], "-agg-depth"),
    (["-agg", "max", "-agg-depth", "0"], "-agg-depth"),
    (["-agg", "noisy-or", "-agg-depth", "2"], "-agg-depth belongs to -agg max"),
    (["-weights", "learned"], "-weights"),
])
def test_command_line_refuses_before_a_miner_exists(args, word, monkeypatch, capsys):
    def no_miner(*a, **k):
        raise AssertionError("the miner was created")
    monkeypatch.setattr(miner_mod, "RuleMiner", no_miner)
    with pytest.raises(SystemExit) as err:
        miner_mod.main(["-data-path", "/nonexistent", "-rule-file", "rules.txt", "-evaluate", "test"] + args)
    assert err.value.code == 2 and word in capsys.readouterr().err


def test_command_line_needs_a_query_for_agg_and_weights(monkeypatch, capsys):
    def no_miner(*a, **k):
        raise AssertionError("the miner was created")
    monkeypatch.setattr(miner_mod, "RuleMiner", no_miner)
    for args in (["-agg", "max"], ["-weights", "conf"]):
        with pytest.raises(SystemExit) as err:
            miner_mod.main(["-data-path", "/nonexistent", "-output-file", "rules.txt"] + args)
        assert err.value.code == 2 and "-agg and -weights" in capsys.readouterr().err


def test_library_exports_set_aggregation_and_refuses_an_unknown_mode():
    L = _native.lib()
    assert hasattr(L, "rnnl_miner_set_aggregation")
    assert "rnnl_miner_set_aggregation" in [n for n, _, _ in _native.SIGNATURES]
    assert (_native.MINER_AGG_SUM, _native.MINER_AGG_NOISY_OR, _native.MINER_AGG_MAX) == (0, 1, 2)
    for agg in (3, -1, 1 << 20):  # decided before the handle is looked at
        assert L.rnnl_miner_set_aggregation(None, agg, 1, None, None) == _native.RNNL_ERR_INVALID
        assert "agg must be" in L.rnnl_last_error().decode()
    for depth in (0, 4, -1):
        assert L.rnnl_miner_set_aggregation(None, _native.MINER_AGG_MAX, depth, None, None) == \
            _native.RNNL_ERR_INVALID
        assert "depth must be 1..3" in L.rnnl_last_error().decode()
    for agg, depth in ((_native.MINER_AGG_SUM, 7), (_native.MINER_AGG_NOISY_OR, 0), (_native.MINER_AGG_MAX, 3)):
        assert L.rnnl_miner_set_aggregation(None, agg, depth, None, None) == _native.RNNL_ERR_INVALID
        assert "bad arguments" in L.rnnl_last_error().decode()  # a known mode goes on to the handle
