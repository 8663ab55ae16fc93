"""CPU side of rule bodies of up to five relations: the argument checks of
rnnl_rule_key_bits / rnnl_rule_search_long / rnnl_miner_set_rules_long (all
come before any device call), the long rule keys of rnnlogic_amd.miner, the
max_body limit of RuleMiner and read_rule_file, and the fixtures of
tools/make_golden_rules_long.py themselves."""
import ctypes
import itertools
import os
import random
import types

import numpy as np
import pytest

from conftest import GOLDEN
from rnnlogic_amd import _native
from rnnlogic_amd import miner as miner_mod


def test_key_bits_and_their_bound():
    L = _native.lib()
    bits = ctypes.c_int32(-1)
    for R, length, want in ((1, 5, 1), (2, 5, 1), (3, 5, 2), (22, 5, 5), (474, 5, 9), (1024, 5, 10), (1025, 4, 11),
                            (4096, 4, 12), (32767, 3, 15), (32767, 1, 15)):
        assert L.rnnl_rule_key_bits(R, length, ctypes.byref(bits)) == _native.RNNL_OK
        assert bits.value == want and 3 + (length + 1) * want <= 64
        assert miner_mod.long_key_bits(R, length) == want
    for R, length, bound in ((1025, 5, "1024"), (4097, 4, "4096"), (32767, 5, "1024")):
        assert L.rnnl_rule_key_bits(R, length, ctypes.byref(bits)) == _native.RNNL_ERR_INVALID
        msg = L.rnnl_last_error().decode()
        assert bound in msg and str(R) in msg and "max_length %d" % length in msg
        with pytest.raises(_native.NativeError) as err:
            miner_mod.long_key_bits(R, length)
        assert err.value.code == _native.RNNL_ERR_INVALID
    for R, length in ((0, 4), (5, 0), (5, 6)):
        assert L.rnnl_rule_key_bits(R, length, ctypes.byref(bits)) == _native.RNNL_ERR_INVALID
    assert L.rnnl_rule_key_bits(5, 4, None) == _native.RNNL_ERR_INVALID


def test_new_entry_points_check_their_arguments_without_a_device():
    L = _native.lib()
    buf = (ctypes.c_uint64 * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # no handle: nothing else is looked at, no device is touched
    assert L.rnnl_rule_search_long(None, 4, 0, p, 1024, p, 0, p, None) == _native.RNNL_ERR_INVALID
    assert b"rnnl_rule_search_long" in L.rnnl_last_error() and b"1..5" in L.rnnl_last_error()
    assert L.rnnl_miner_set_rules_long(None, p, p, p, None) == _native.RNNL_ERR_INVALID
    assert b"rnnl_miner_set_rules_long" in L.rnnl_last_error()
    assert L.rnnl_miner_set_rules(None, p, p, p, None) == _native.RNNL_ERR_INVALID
    assert b"rnnl_miner_set_rules:" in L.rnnl_last_error()
    assert L.rnnl_rule_search(None, 4, p, 1024, p, 0, p, None) == _native.RNNL_ERR_INVALID  # as before


def test_long_keys_round_trip_and_sort_as_the_reference():
    rng = random.Random(3)
    for R, length in ((1, 4), (2, 5), (7, 5), (22, 5), (474, 5), (1024, 5), (4096, 4), (1025, 4)):
        rules = set()
        for hd in (0, R // 2, R - 1):
            rules.add((hd, ()))
            for n in range(1, length + 1):
                rules.add((hd, (R - 1,) * n))
                rules.add((hd, (0,) * n))
                for _ in range(6):
                    rules.add((hd, tuple(rng.randrange(R) for _ in range(n))))
        rules = list(rules)
        rng.shuffle(rules)
        keys = miner_mod.encode_long(rules, R, length)
        assert keys.dtype == np.uint64 and len(set(keys.tolist())) == len(rules)
        assert not np.any(keys == np.uint64(0xFFFFFFFFFFFFFFFF))  # the empty slot of the device set
        want = sorted(rules, key=lambda x: (x[0], len(x[1]), x[1]))  # std::set<Rule> order per head
        assert miner_mod.RuleMiner.decode(keys, R, length) == want
        head, ln, body = miner_mod.unpack_long(keys, R, length)
        assert body.shape == (len(rules), length)
        for i, (hd, b) in enumerate(rules):
            assert (int(head[i]), int(ln[i])) == (hd, len(b))
            assert tuple(body[i, :len(b)].tolist()) == b and not body[i, len(b):].any()
    with pytest.raises(ValueError):
        miner_mod.encode_long([(0, (1, 1, 1, 1, 1))], 3, 4)


def test_decode_of_the_short_keys_is_unchanged():
    rules = [(0, (1,)), (0, (2, 3)), (5, (32766, 0, 7)), (32766, (1, 2, 3))]
    keys = np.asarray([(hd << 47) | (len(b) << 45) | sum(x << s for x, s in zip(b, (30, 15, 0))) for hd, b in rules],
                      dtype=np.uint64)
    assert miner_mod.RuleMiner.decode(keys[::-1]) == rules
    assert miner_mod.RuleMiner.decode(keys, 32767, 3) == rules


def test_read_rule_file_max_body(tmp_path):
    f = tmp_path / "rules.txt"
    f.write_text("1 0 2 1 0 2 0.25\n0 1 1 1 1 -0.5\n2\n1 0 0 0 0 0\n")
    rules, weights = miner_mod.read_rule_file(str(f), 3, max_body=5)
    assert rules == [[(0, (1, 1, 1, 1))], [(1, (0, 2, 1, 0, 2)), (1, (0, 0, 0, 0, 0))], [(2, ())]]
    assert weights == [[-0.5], [0.25, 0.0], [0.0]]
    with pytest.raises(ValueError) as err:
        miner_mod.read_rule_file(str(f), 3, max_body=4)
    assert "max_body" in str(err.value) and "rules.txt:1" in str(err.value)
    for default in (dict(), dict(max_body=3)):
        with pytest.raises(ValueError) as err:
            miner_mod.read_rule_file(str(f), 3, **default)
        assert "at most 3 relations" in str(err.value) and "max_body" in str(err.value)
    f.write_text("1 0 2 1 0 2 1 0.25\n")  # six relations
    with pytest.raises(ValueError) as err:
        miner_mod.read_rule_file(str(f), 3, max_body=5)
    assert "at most 5 relations" in str(err.value)
    f.write_text("1 0 2 1 0.25\n")
    assert miner_mod.read_rule_file(str(f), 3) == ([[], [(1, (0, 2, 1))], []], [[], [0.25], []])
    for bad in (2, 6, None, "5"):
        with pytest.raises(ValueError):
            miner_mod.read_rule_file(str(f), 3, max_body=bad)


def bare_miner(n_relations, **attrs):
    m = object.__new__(miner_mod.RuleMiner)
    m._rule_off = np.zeros(n_relations + 1, dtype=np.int32)
    m.graph = types.SimpleNamespace(relation_size=n_relations, entity_size=5)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def test_max_body_is_a_class_attribute_and_governs_every_door(tmp_path):
    assert miner_mod.RuleMiner.max_body == 3 and "max_body" not in vars(bare_miner(3))
    long_rule = [[(0, (1, 1, 1, 1))], [], []]
    f = tmp_path / "rules.txt"
    f.write_text("0 1 1 1 1 0.5\n")
    for m, limit in ((bare_miner(3), 3), (bare_miner(3, max_body=4), 4)):
        rules = [[(0, (1,) * (limit + 1))], [], []]
        for call in (lambda: m.search(limit + 1), lambda: m.search_keys(limit + 1),
                     lambda: m.mine(limit + 1, 1, 0, 0, 0.01, 0.0, 100.0), lambda: m.set_logic_rules(rules)):
            with pytest.raises(ValueError) as err:
                call()
            assert "at most %d relations" % limit in str(err.value) and "max_body" in str(err.value)
    with pytest.raises(ValueError):
        bare_miner(3).set_logic_rules(long_rule)
    with pytest.raises(ValueError):
        bare_miner(3).read_rules(str(f))
    with pytest.raises(ValueError) as err:
        bare_miner(3, max_body=5).set_logic_rules([[(0, (1,) * 6)], [], []])
    assert "at most 5 relations" in str(err.value) and "max_body" not in str(err.value)
    for bad in (2, 6, 3.5):
        with pytest.raises(ValueError):
            miner_mod.RuleMiner(types.SimpleNamespace(), max_body=bad)
    # the key bound is met before anything is allocated
    with pytest.raises(_native.NativeError) as err:
        bare_miner(1025, max_body=5).search_keys(5)
    assert err.value.code == _native.RNNL_ERR_INVALID and "1024" in str(err.value)


def load_pool(z, length):
    flat, rules, k = z["flat%d" % length].astype(np.int64), [], 0
    while k < len(flat):
        rules.append((int(flat[k]), tuple(int(x) for x in flat[k + 2:k + 2 + flat[k + 1]])))
        k += 2 + int(flat[k + 1])
    return rules


def test_fixtures_are_data_and_consistent():
    names = sorted(f for f in os.listdir(GOLDEN) if f.startswith("_rules_long_") and f.endswith(".npz"))
    assert len(names) == 10
    for f in names:
        assert os.path.getsize(os.path.join(GOLDEN, f)) < 300 * 1024
        z = np.load(os.path.join(GOLDEN, f), allow_pickle=False)
        if f == "_rules_long_umls_L4.npz":
            assert int(z["count"]) == 501799 and z["per_len"].tolist() == [190, 2863, 36230, 462516]
            assert len(str(z["sha256"])) == 64
            continue
        tri, E, R = z["triples"], int(z["E"]), int(z["R"])
        assert tri.shape[1] == 3 and tri.min() >= 0 and tri[:, [0, 2]].max() < E and tri[:, 1].max() < R
        p4, p5 = load_pool(z, 4), load_pool(z, 5)
        assert p4 == sorted(set(p4), key=lambda x: (x[0], len(x[1]), x[1])) and max(len(b) for _, b in p4) <= 4
        assert [x for x in p5 if len(x[1]) <= 4] == p4 and any(len(b) == 5 for _, b in p5)
        loops = sorted(set(int(r) for h, r, t in tri if h == t))
        assert [hd for hd, b in p5 if not b] == loops  # one body-less rule per relation with a self-loop triple
        assert all(all(0 <= x < R for x in b) for _, b in itertools.chain(p4, p5))
